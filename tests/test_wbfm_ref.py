"""tests/wbfm_ref.py (the float64 reference of the per-sample WBFM tests) checked on the
CPU against the C oracle: the f64 stages agree with the oracle's stage functions and with
oracle.wbfm within the stage bounds, per input class and call split; the guard condition
holds on every input test_gpu_wbfm_exact.py uses; faults planted in the oracle's output
push rho above MARGIN rho(oracle) (one of them with a whole-output nrmse below 1e-5, the
figure test_gpu_parity.py asserts); and the split-f16 term of B is needed, not slack."""
import numpy as np
import pytest

import fir_ref as FR
import iir_ref as IR
import wbfm_ref as W
from conftest import nrmse, wbfm_input

MARGIN = 5.0   # as tests/test_gpu_wbfm_exact.py
N = W.N_MAIN
SPLITS = {"one call": lambda n: [n], "ragged": W.ragged, "8192s": W.even}


def test_geometry_restated():
    """kernels.hpp / k_wbfm.hip / blocks.cpp as wbfm_ref restates them."""
    assert (W.M, W.TILE, W.TILE_IN, W.K_SG_L, W.K_FU_TAIL) == (8, 128, 1024, 1024, 128)
    assert (W.CLAMP_BELOW, W.REFRESH, W.K_BACK_A, W.K_BACK_W, W.SEG_HORIZON) == (2048, 64, 4096, 510, 896)
    assert W.FRONT_PER_CU == min((160 * 1024) // (8 * (128 + 16 + 2) * 8), 12) & ~3 == 12
    # 4 * 8192 + 5: five sub-ranges, the last with one output; max_segments 1, 2, 3, 5
    nd = W.n_out(N)
    assert nd == 4 * 1024 + 1
    assert [W.seg_plan(nd, 1, s, 512) for s in (1, 2, 3, 5)] == [(1, 5120), (2, 3072), (3, 2048), (5, 1024)]
    # a 73rd tile in one segment crosses the n & 63 refresh
    assert W.seg_plan(W.n_out(9 * 8192 + 5), 1, 1, 512)[1] // W.TILE > W.REFRESH
    # the front wave ranges: N 128 - 1 phi
    assert W.front2_plan(4097, 1, 256) == (1, 127, 33)
    assert W.front2_plan(W.N2_NDEC, W.N2_NCH, 256)[0] == 2
    # the dropout starts mid-tile and ends in another sub-range
    assert (W.DROP_AT // 8) % W.TILE not in (0, W.TILE - 1) and W.DROP_AT % 8
    assert (W.DROP_AT // 8) // W.K_SG_L != ((W.DROP_AT + W.DROP_LEN) // 8) // W.K_SG_L


def test_atan2_64_is_the_approximant(oracle):
    rng = np.random.default_rng(W.seed_of("atan"))
    y, x = rng.standard_normal(4096).astype(np.float32), rng.standard_normal(4096).astype(np.float32)
    y[:4], x[:4] = [0, 0, 1, -1], [0, -1, 0, 0]
    ref = np.array([oracle.atan2_approx(float(a), float(b)) for a, b in zip(y, x)])
    got = W.atan2_64(y.astype(np.float64), x.astype(np.float64))
    assert got[0] == 0.0
    assert np.max(np.abs(got - ref)) <= 8 * W.U * np.pi


def _tb(oracle, cls, split, **kw):
    x = W.stream(oracle, wbfm_input, cls, N)
    lens = SPLITS[split](N)
    T = W.cached(("T", cls, N, split, tuple(sorted(kw.items()))), lambda: W.truth_bound(oracle, x, lens, **kw))
    return x, lens, T


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("cls", W.CLASSES)
def test_stages_agree_with_the_oracle(oracle, cls, split):
    """Per stage: |oracle's f32 stage - f64 stage| within the stage's bound, the whole
    chain within B (rho(oracle) <= 1), and the stage composition is oracle.wbfm's bits."""
    x, lens, T = _tb(oracle, cls, split)
    mixed, d, f, y = W.oracle_run(oracle, x, lens, stages=True)
    if split == "one call":
        assert np.array_equal(y, oracle.wbfm(x))
    if split == "8192s":
        assert np.array_equal(y, oracle.wbfm(x, chunk=W.SUB_IN))
    assert len(y) == len(T.y) == sum(T.out_lens)
    assert np.all(np.abs(mixed.astype(np.complex128) - T.z) <= W.C_MIX * W.U * np.abs(T.z))   # the phasors are data
    assert np.all(np.abs(d.astype(np.complex128) - T.d) <= T.e_d)
    r_f, i_f = IR.rho(f.astype(np.float64), T.f, T.e_f)
    r, i = W.rho(y, T)
    print(f"[parity] wbfm_ref {cls} {split}: rho(oracle) {r:.3e} at {i}, LpCascade stage {r_f:.3e} at {i_f}, "
          f"nrmse {nrmse(y, T.y):.3e}")
    assert r_f <= 1.0 and r <= 1.0
    if cls == "zero":
        assert not y.any() and not T.y.any() and not T.B.any()
    else:
        assert r > 0


def test_direct_convolution_leaves_exact_zeros(oracle):
    """The truth before the first sample's response is exactly zero (no FFT residue), and a
    dropout's q = 0 samples give phi exactly 0."""
    x, lens, T = _tb(oracle, "dropout", "one call")
    z = np.flatnonzero(T.q == 0)
    assert len(z) > 2000 and not T.phi[z].any() and not T.e_phi[z].any()
    x0 = x.copy()
    x0[:4096] = 0
    T0 = W.truth_bound(oracle, x0)
    assert not T0.y[:512].any() and not T0.B[:512].any() and T0.y[520] != 0


def _committed(oracle):
    """Every (label, input, calls, reset points) test_gpu_wbfm_exact.py runs."""
    for cls in W.CLASSES:
        x = W.stream(oracle, wbfm_input, cls, N)
        for sp, fn in SPLITS.items():
            yield f"{cls} {sp}", x, fn(N), W.resets(cls), {}
    for n in W.SEG_LENGTHS + W.SPLIT_LENGTHS + [W.N_BIG]:
        yield f"default n={n}", W.stream(oracle, wbfm_input, "default", n), [n], [0], {}
    for c, fo in enumerate(W.CH_OFFS):
        yield f"channel {c}", W.stream(oracle, wbfm_input, "default", N, f_off=fo, tag=f"-ch{c}"), [N], [0], dict(f_off=fo)
    for c in range(W.N2_NCH):
        yield (f"N=2 channel {c}", W.stream(oracle, wbfm_input, "default", 8 * W.N2_NDEC, tag=f"-n2-{c}"), [8 * W.N2_NDEC],
               [0], {})
    yield "m=10", W.stream(oracle, wbfm_input, "default", N), [N], [0], dict(m=10)
    yield "seek", W.stream(oracle, wbfm_input, "default", W.SEEK_N, tag="-seek"), [W.SEEK_N], [0], dict(k0=W.SEEK_K0)


def test_guard_condition(oracle):
    """At most 4 samples per stream within GUARD e_q of a discontinuity of the approximant,
    and only within 16 decimated outputs after a reset or a dropout edge."""
    worst = np.inf
    for label, x, lens, resets, kw in _committed(oracle):
        T = W.truth_bound(oracle, x, lens, **kw)
        trip = T.tripped
        g = T.guard[np.isfinite(T.guard)]
        m = int(kw.get("m", 8))
        rs = [r * 8 // m for r in resets]
        far = [int(j) for j in trip if not any(0 <= j - r <= 16 for r in rs)]
        if len(trip) or (len(g) and g.min() < 100):
            print(f"[guard] {label}: {len(trip)} tripped at {trip.tolist()}, min guard {g.min() if len(g) else np.inf:.3g}")
        assert len(trip) <= 4 and not far, (label, trip, far)
        if len(g):
            worst = min(worst, float(np.min(np.where(T.guard < W.GUARD, np.inf, T.guard))))
    print(f"[guard] smallest guard that does not trip: {worst:.3g}")


# ---- planted faults ---------------------------------------------------------------------
def _after_phi(T, phi, a):
    return np.convolve(IR.lp4_64(phi, T.coef), a)[:len(phi)]


def _faults(oracle, x, T):
    """name -> the truth with one fault planted (f64); the fault is added to the oracle's output."""
    d = T.design
    h_dec, h_aud = W._taps_default(oracle, d)
    a = FR.standard_taps(h_aud).astype(np.float64)
    g = FR.standard_taps(h_dec).astype(np.float64)
    e = W.K_SG_L   # a sub-range edge
    out = {}
    y = T.y.copy()
    y[e] += 1e-4 * np.sqrt(np.mean(T.y ** 2))
    out["one output at a sub-range edge moved by 1e-4 rms"] = y
    # the FIR history of sub-range 1 taken from an f16 hi-only reconstruction
    f = T.f.copy()
    sc = 2.0 ** (15 - np.frexp(np.abs(f[e - 128:e + 1024]).max())[1])
    fh = f.copy()
    fh[e - 128:e] = (f[e - 128:e] * sc).astype(np.float16).astype(np.float64) / sc
    y = T.y.copy()
    y[e:e + 1024] = np.convolve(fh, a)[e:e + 1024]
    out["FIR history from an f16 hi-only reconstruction at one sub-range edge"] = y
    sa = 2.0 ** (15 - np.frexp(np.abs(a).max())[1])
    out["audio taps hi part only"] = np.convolve(T.f, (a * sa).astype(np.float16).astype(np.float64) / sa)[:len(T.f)]
    f0 = np.concatenate([IR.lp4_64(T.phi[:2 * e], T.coef), IR.lp4_64(T.phi[2 * e:], T.coef)])
    out["IIR restarted from zero state at output 2048"] = np.convolve(f0, a)[:len(f0)]
    # tile 9's first FIR windows read the halo of the tile before the previous one
    p = IR.phasors(oracle, len(x), -float(np.float32(d["f_off"])), d["fs"]).astype(np.complex128)
    z = x.astype(np.complex128) * p
    s = 9 * W.TILE_IN
    zs = z.copy()
    zs[s - 17 * 8:s] = z[s - 17 * 8 - W.TILE_IN:s - W.TILE_IN]
    idx = W._kept([len(x)], 8)
    ds = T.d.copy()
    t = slice(9 * W.TILE, 10 * W.TILE)
    ds[t] = W._fir_at(zs, g, idx[t])
    k = float(np.float32(np.float32(1.0) / np.float32(d["dev_hz"])))
    qs = ds * np.conj(np.concatenate([[1.0 + 0.0j], ds[:-1]]))
    out["a stale 17-column halo at one tile edge"] = _after_phi(T, W.atan2_64(qs.imag, qs.real) * k, a)
    return out


def test_planted_faults_are_seen(oracle):
    x, lens, T = _tb(oracle, "default", "one call")
    y = W.oracle_run(oracle, x).astype(np.float64)
    r0, i0 = W.rho(y, T)
    print(f"[fault] oracle: rho {r0:.3e} at {i0}")
    for name, yt in _faults(oracle, x, T).items():
        bad = y + (yt - T.y)
        r, i = W.rho(bad, T)
        e = nrmse(bad, y)
        print(f"[fault] {name}: whole-output nrmse {e:.2e}, rho {r:.3e} at {i} = {r / r0:.3g} x the oracle's")
        assert r > MARGIN * r0, name
        if name.startswith("one output"):
            assert e < 1e-5   # the figure test_gpu_parity.py asserts does not see it


@pytest.mark.parametrize("cls", ["step", "dropout"])
def test_f16_term_is_needed(oracle, cls):
    """A numpy model of sg::back's split-f16 audio FIR on the oracle's own f32 LpCascade
    output f, judged where a model of the FIR can be judged: against the f64 FIR of the same
    f and the audio stage's own terms of B (e_f = 0), with the oracle's f32 FirLowpass of the
    same f as the yardstick. With the f16 term the model is within MARGIN rho(oracle), without
    it outside: the model leaves the K-term bound while f ramps up from zero and by orders of
    magnitude inside the dropout, where |f| has decayed and the sub-range's scale has not.
    Through the whole chain's B the model passes either way (printed): there the
    discriminator's bound is ~1e3 times the audio stage's."""
    x, lens, T = _tb(oracle, cls, "one call")
    _, _, T0 = _tb(oracle, cls, "one call", f16=False)
    _, _, f, y = W.oracle_run(oracle, x, stages=True)
    a = FR.standard_taps(W._taps_default(oracle, T.design)[1])
    ym = W.f16_fir_model(f, a, T.out_lens)
    assert W.rho(ym, T)[0] <= MARGIN * W.rho(y, T)[0]
    print(f"[f16] {cls} whole chain: model {W.rho(ym, T)[0]:.3e} / oracle {W.rho(y, T)[0]:.3e} with the term, "
          f"{W.rho(ym, T0)[0]:.3e} / {W.rho(y, T0)[0]:.3e} without")
    t, b1 = W.fir_stage(f, a, True)
    _, b0 = W.fir_stage(f, a, False)
    (r_m, i_m), (r_o, _) = IR.rho(ym, t, b1), IR.rho(y.astype(np.float64), t, b1)
    (r_m0, i_m0), (r_o0, _) = IR.rho(ym, t, b0), IR.rho(y.astype(np.float64), t, b0)
    print(f"[f16] {cls} audio stage: with the term model {r_m:.3e} at {i_m} / oracle {r_o:.3e}; without it model "
          f"{r_m0:.3e} at {i_m0} / oracle {r_o0:.3e}")
    assert r_m <= 1.0 and r_m <= MARGIN * r_o
    assert r_m0 > MARGIN * r_o0


def test_mean_step_jitter(oracle):
    """What test_gpu_wbfm_exact.MARGINS' carrier entries rest on: an f64 chain that differs
    from the truth by the mean-step phasor alone sits at 1.3e-4 of B (output 1527) on any
    input. That is 1 % of the oracle's rho on the default signal and 13.6 x the oracle's on
    the silent noise-free carrier, where the oracle only rounds a constant."""
    for cls, lo, hi in (("carrier", 10.0, 20.0), ("default", 0.0, 0.05)):
        x, lens, T = _tb(oracle, cls, "one call")
        y, jit = W.mean_step_chain(oracle, x, T)
        (r, i), (r_o, _) = W.rho(y, T), W.rho(W.oracle_run(oracle, x), T)
        print(f"[jitter] {cls}: phase jitter <= {jit:.2e} rad, rho {r:.3e} at {i} = {r / r_o:.3g} x the oracle's {r_o:.3e}")
        assert jit < 1e-5 and lo <= r / r_o <= hi


def test_edge_designs_sit_on_their_sides(oracle):
    E = W.edge_designs(oracle)
    print("[edge]", {k: (round(v[0], 2), v[1], v[2]) for k, v in E.items()})
    assert E["seg_in"][1] and not E["seg_out"][1]
    assert E["split_in"][2] and not E["split_out"][2]
    A = W.lp4_A(oracle, W.C2["audio_bw"])
    assert IR.fro(A, W.SEG_HORIZON) < W.SEG_TRUNC and IR.fro(A, W.K_BACK_W) < W.SPLIT_TRUNC  # the defaults: both fused paths
