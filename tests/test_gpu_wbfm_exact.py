"""Per-sample tests of the WBFM chain kernels (csrc/k_wbfm.hip): k_wbfm_seg, k_wbfm_front2 +
k_wbfm_back, and the graph path, at every seam.

Each run is compared, sample for sample, with the float64 truth of tests/wbfm_ref.py
(validated against the C oracle in tests/test_wbfm_ref.py) through one figure,

    rho(y) = max_n |y[n] - truth[n]| / B[n],

B the a-priori bound of wbfm_ref.truth_bound, computed from truth
quantities only; where B is exactly 0 the output must be exactly 0. What is asserted is
rho(gpu) <= MARGIN rho(oracle): the oracle's own f32 run of the same calls against the same
truth and B. MARGIN = 5 is the project's margin (test_gpu_scan_exact.py, ssb_tol). Every case
prints `[parity] ... rho gpu / oracle` with the sample index of each, the GPU's also as
(segment, sub-range, tile, offset) or (front wave, tile, offset; back workgroup, half,
offset), so that the seam at fault can be read off the log. The geometry is restated in
wbfm_ref and asserted here against kernels.hpp / k_wbfm.hip / blocks.cpp.
"""
import numpy as np
import pytest

import wbfm_ref as W
from conftest import wbfm_input

pytestmark = pytest.mark.gpu

# kernels.hpp:95, 160, 118, 101, 103; k_wbfm.hip Fw<2>::TW / NEW, launch_wbfm_seg (clamp = n < 2 NEW),
# k_wbfm_seg ((n & 63) == 0), front2_plan<2> (per_cu); blocks.cpp build_fused (kSgL - 128, 1e-10; kBackW, 1e-7)
assert (W.M, W.K_SG_L, W.K_FU_TAIL, W.K_BACK_A, W.K_BACK_W) == (8, 1024, 128, 4096, 510)
assert (W.TILE, W.TILE_IN, W.CLAMP_BELOW, W.REFRESH, W.FRONT_PER_CU) == (128, 1024, 2048, 64, 12)
assert (W.SEG_HORIZON, W.SEG_TRUNC, W.SPLIT_TRUNC) == (896, 1e-10, 1e-7)

MARGIN = 5.0
# case label prefix -> margin, each justified in DESIGN.md §3.5 (at most 1.5 x the measured ratio)
MARGINS = {
    # The silent noise-free carrier is the one input on which the reference does nothing but
    # round a constant (rho 9.7e-6, two orders below every other class). The fused paths mix
    # with the closed-form phasor of the recurrence's mean step, the truth
    # with the recurrence's own phasors: their difference, a jitter of 5.5e-6 rad at most, is
    # 1.3e-4 of B at output 1527 in an otherwise exact f64 chain (test_wbfm_ref.py
    # test_mean_step_jitter: 13.6 x the oracle's rho). Measured 12.9 (one call, every segment
    # count, 8192s), 14.7 (ragged), 14.7 (split), all at outputs 1528 - 1530 whatever the
    # geometry; the graph path, which runs the Rotator block, is not affected.
    "segmented carrier ragged": 20.0,
    "segmented carrier": 18.0,
    "split carrier": 20.0,
}
N = W.N_MAIN
SPLITS = {"one call": lambda n: [n], "ragged": W.ragged, "8192s": W.even}


def margin_of(label):
    for k, v in MARGINS.items():
        if label.startswith(k):
            return v
    return MARGIN


def make(lib, path="auto", max_seg=0, **design):
    return lib.WbfmChain(**design).configure(path, max_seg)


def run_calls(blk, x, lens):
    outs, i = [], 0
    for n in lens:
        outs.append(blk.process(np.ascontiguousarray(x[..., i:i + n])))
        i += n
    return np.concatenate(outs, axis=-1)


def lib_taps(blk, oracle, design):
    """The taps the library reports, asserted equal to the oracle's."""
    t = (np.asarray(blk.taps(0), np.float32), np.asarray(blk.taps(1), np.float32))
    o = W._taps_default(oracle, W.design(**design))
    assert np.array_equal(t[0], o[0]) and np.array_equal(t[1], o[1])
    return t


def reference(oracle, blk, key, x, lens, path, k0=0, **design):
    """(truth and B, the oracle's own output) of the calls, one computation per key."""
    bpath = path if path in ("split", "graph") else "segmented"
    taps = lib_taps(blk, oracle, design)
    T = W.cached(("T", key, tuple(lens), bpath, k0, tuple(sorted(design.items()))),
                 lambda: W.truth_bound(oracle, x, lens, path=bpath, k0=k0, taps=taps, **design))
    yo = W.cached(("O", key, tuple(lens), k0, tuple(sorted(design.items()))),
                  lambda: W.oracle_run(oracle, x, lens, k0=k0, **design))
    return T, yo


def judge(label, got, T, yo, path, cut=None, **geo):
    """Print the rho pair and where each sits; assert rho(gpu) <= margin rho(oracle)."""
    ty, tb = (T.y, T.B) if cut is None else (T.y[:cut], T.B[:cut])
    yo = yo if cut is None else yo[:cut]
    assert got.shape == ty.shape, (label, got.shape, ty.shape)
    r_g, i_g = W.IR.rho(np.asarray(got, np.float64), ty, tb)
    r_o, i_o = W.IR.rho(np.asarray(yo, np.float64), ty, tb)
    m = margin_of(label)
    ratio = r_g / r_o if r_o > 0 else (0.0 if r_g == 0 else np.inf)
    print(f"[parity] wbfm exact {label}: rho gpu {r_g:.3e} at {i_g} [{W.where_stream(i_g, T.out_lens, path, **geo)}] / "
          f"oracle {r_o:.3e} at {i_o} = {ratio:.3g} (margin {m:g})")
    assert r_g <= m * r_o, f"{label}: rho gpu {r_g:.3e} at {i_g} > {m:g} x oracle {r_o:.3e}"
    return ratio


def case(lib, oracle, label, cls, n, lens, path, max_seg=0, tag="", **design):
    x = W.stream(oracle, wbfm_input, cls, n, f_off=design.get("f_off", W.C2["f_off"]), tag=tag)
    blk = make(lib, path, max_seg, **design)
    T, yo = reference(oracle, blk, (cls, n, tag), x, lens, path, **design)
    got = run_calls(blk, x, lens)
    judge(label, got, T, yo, path, max_segments=max_seg, ncu=lib.device_cus())
    return blk, x, got


# ------------------------------------------------------------------ segmented path ==
@pytest.mark.parametrize("n", W.SEG_LENGTHS)
def test_segmented_one_call_lengths(gpu_lib, oracle, n):
    """k_wbfm_seg at every length around a tile, the CLAMP threshold (2,048 inputs) and a
    sub-range, up to five sub-ranges with one output in the last (resident default)."""
    case(gpu_lib, oracle, f"segmented n={n}", "default", n, [n], "segmented")


@pytest.mark.parametrize("max_seg", [1, 2, 3, 5])
def test_segmented_segment_counts(gpu_lib, oracle, max_seg):
    """4 * 8192 + 5 in segments of 5, 3 + 2, 2 + 2 + 1 and 1 sub-range each: every hand-off
    (zero-state end state, published record, deferred first sub-range)."""
    assert W.seg_plan(W.n_out(N), 1, max_seg, 1 << 20) == {1: (1, 5120), 2: (2, 3072), 3: (3, 2048), 5: (5, 1024)}[max_seg]
    case(gpu_lib, oracle, f"segmented max_segments={max_seg}", "default", N, [N], "segmented", max_seg)


def test_segmented_phasor_refresh(gpu_lib, oracle):
    """One segment of 9 * 8192 + 5 inputs: its 73 tiles cross the (n & 63) == 0 refresh of
    the tile phasors."""
    assert W.seg_plan(W.n_out(W.N_BIG), 1, 1, 1 << 20)[1] // W.TILE > W.REFRESH
    case(gpu_lib, oracle, "segmented one segment of 73 tiles", "default", W.N_BIG, [W.N_BIG], "segmented", 1)


@pytest.mark.parametrize("max_seg", [2, 0])
@pytest.mark.parametrize("cls", W.CLASSES[1:])
def test_segmented_input_classes(gpu_lib, oracle, cls, max_seg):
    """Quiet audio, a silent carrier, deep fades, RF at 1e-3 and 1e-6 (|q| far below the
    approximant's eps), a dropout of exact zeros (phi exactly 0, the LpCascade through the
    subnormals, a vanishing f16 scale), a loud-to-quiet step on a sub-range edge, all zeros."""
    _, _, got = case(gpu_lib, oracle, f"segmented {cls} max_segments={max_seg}", cls, N, [N], "segmented", max_seg)
    if cls == "zero":
        assert not got.any()


@pytest.mark.parametrize("split", ["ragged", "8192s"])
@pytest.mark.parametrize("cls", W.CLASSES)
def test_segmented_streaming(gpu_lib, oracle, cls, split):
    """The same streams in calls that cut mid-tile at a length that is no multiple of 8, on
    a sub-range edge, and below the 128-sample history; the truth is the one of the same
    calls, the oracle's rho the whole stream's."""
    case(gpu_lib, oracle, f"segmented {cls} {split}", cls, N, SPLITS[split](N), "segmented")


# ---------------------------------------------------------------------- split path ==
@pytest.mark.parametrize("split", ["one call", "ragged"])
@pytest.mark.parametrize("n", W.SPLIT_LENGTHS)
def test_split_lengths(gpu_lib, oracle, n, split):
    """k_wbfm_front2 + k_wbfm_back around a front wave's range (N 128 - 1 phi), a back half
    (2,048), a back workgroup (kBackA = 4,096) and one and a half of them, in one call and
    streamed."""
    case(gpu_lib, oracle, f"split n={n} {split}", "default", n, SPLITS[split](n), "split")


@pytest.mark.parametrize("cls", W.CLASSES[1:])
def test_split_input_classes(gpu_lib, oracle, cls):
    _, _, got = case(gpu_lib, oracle, f"split {cls}", cls, N, [N], "split")
    if cls == "zero":
        assert not got.any()


def test_split_front_wave_walks_two_tiles(gpu_lib, oracle):
    """N = 2 in front2_plan: 8 channels of 385 tiles each are more tiles than the device has
    front waves (12 per CU), so every wave walks two and carries the halo across."""
    ncu = gpu_lib.device_cus()
    N2, L, wpc = W.front2_plan(W.N2_NDEC, W.N2_NCH, ncu)
    assert N2 == 2, (ncu, N2)
    n = 8 * W.N2_NDEC
    xs = [W.stream(oracle, wbfm_input, "default", n, tag=f"-n2-{c}") for c in range(W.N2_NCH)]
    blk = gpu_lib.WbfmChain(f_off=[W.C2["f_off"]] * W.N2_NCH).configure("split")
    got = blk.process(np.stack(xs))
    for c in (0, 3, W.N2_NCH - 1):
        T, yo = reference(oracle, blk, ("default", n, f"-n2-{c}"), xs[c], [n], "split")
        judge(f"split N=2 channel {c}", got[c], T, yo, "split", nch=W.N2_NCH, ncu=ncu)


# ------------------------------------------------------------------ validity edges ==
@pytest.mark.parametrize("name", ["seg_in", "seg_out", "split_in", "split_out"])
def test_validity_edges(gpu_lib, oracle, name):
    """Designs bisected on audio_bw to just inside / outside seg_ok (||A^896|| < 1e-10) and
    split_ok (||A^510|| < 1e-7): configure raises on the wrong side, auto gives the bits of
    the path it must resolve to, and every valid fused path is within its B with one
    sub-range per segment (the largest hand-off truncation)."""
    bw, seg_ok, split_ok = W.edge_designs(oracle)[name]
    assert (seg_ok, split_ok) == {"seg_in": (True, False), "seg_out": (False, False), "split_in": (True, True),
                                  "split_out": (True, False)}[name]
    x = W.stream(oracle, wbfm_input, "default", N)
    outs = {}
    for path, ok in (("segmented", seg_ok), ("split", split_ok)):
        if not ok:
            with pytest.raises(gpu_lib.OrionError):
                make(gpu_lib, path, audio_bw=bw)
            continue
        blk = make(gpu_lib, path, 5, audio_bw=bw)
        T, yo = reference(oracle, blk, ("default", N, ""), x, [N], path, audio_bw=bw)
        outs[path] = blk.process(x)
        judge(f"edge {name} {path}", outs[path], T, yo, path, max_segments=5, ncu=gpu_lib.device_cus())
    want = "segmented" if seg_ok else "split" if split_ok else "graph"
    if want == "graph":
        outs["graph"] = make(gpu_lib, "graph", audio_bw=bw).process(x)
        T, yo = reference(oracle, make(gpu_lib, "graph", audio_bw=bw), ("default", N, ""), x, [N], "graph", audio_bw=bw)
        judge(f"edge {name} graph", outs["graph"], T, yo, "graph")
    auto = make(gpu_lib, "auto", 5, audio_bw=bw).process(x)
    assert np.array_equal(auto.view(np.uint32), outs[want].view(np.uint32)), f"auto is not {want}"


# ---------------------------------------------------------------------- graph path ==
@pytest.mark.parametrize("split", ["one call", "ragged"])
@pytest.mark.parametrize("cls,design", [("default", {}), ("carrier", {}), ("zero", {}), ("default", {"m": 10})],
                         ids=["default", "carrier", "zero", "m10"])
def test_graph_path(gpu_lib, oracle, cls, design, split):
    """The four blocks through HBM: the default design (the carrier too: this path mixes
    with the reference's own phasors and needs no margin there), and m = 10 (no fused path)."""
    if design:
        for fused in ("segmented", "split"):
            with pytest.raises(gpu_lib.OrionError):
                make(gpu_lib, fused, **design)
    label = f"graph {cls}{' m=10' if design else ''} {split}"
    _, x, got = case(gpu_lib, oracle, label, cls, N, SPLITS[split](N), "graph", **design)
    if design:  # auto has nothing else to resolve to
        auto = run_calls(make(gpu_lib, "auto", **design), x, SPLITS[split](N))
        assert np.array_equal(auto.view(np.uint32), got.view(np.uint32))
    if cls == "zero":
        assert not got.any()


# ---------------------------------------------------------- alignment and capacity ==
CANARY = 12345.0


@pytest.mark.parametrize("what", ["unaligned-in", "odd-batch", "offset-out", "cap-above", "cap-below"])
@pytest.mark.parametrize("n", [1500, N])
@pytest.mark.parametrize("path", ["segmented", "split"])
def test_alignment_and_capacity(gpu_lib, oracle, path, n, what):
    """process_device: an 8-byte aligned input (the non-A16 kernels), a batch with an odd
    row stride, an output offset by one float (the scalar-store branch of sg::back), and an
    output capacity above and below ceil(n / 8). The output buffer is pre-filled with a
    canary: every float past min(ceil(n / 8), cap) must be unchanged."""
    import torch

    batch = what == "odd-batch"
    n = n - 1 + (n & 1) if batch else n   # odd
    rows = ["default", "quiet"] if batch else ["default"]
    xs = [W.stream(oracle, wbfm_input, c, n) for c in rows]
    nd = W.n_out(n)
    cap = {"cap-above": nd + 7, "cap-below": nd - max(3, nd // 4)}.get(what, nd)
    off = 1 if what == "offset-out" else 0
    blk = (gpu_lib.WbfmChain(f_off=[W.C2["f_off"]] * 2) if batch else gpu_lib.WbfmChain()).configure(path)
    if what == "unaligned-in":
        xb = torch.zeros(n + 1, dtype=torch.complex64, device="cuda")
        xb[1:] = torch.from_numpy(xs[0]).cuda()
        xd = xb[1:]
        assert xd.data_ptr() % 16 == 8
    else:
        xd = torch.from_numpy(np.stack(xs) if batch else xs[0]).cuda()
    buf = torch.full((off + len(rows) * cap + 64,), CANARY, dtype=torch.float32, device="cuda")
    out = buf[off:off + len(rows) * cap]
    out = out.view(len(rows), cap) if batch else out
    assert (out.data_ptr() % 16 == 4) == (off == 1)
    res = blk.process_device(xd, out)
    torch.cuda.synchronize()
    blk.status()
    w = min(nd, cap)
    assert res.shape[-1] == w
    got = buf.cpu().numpy()
    body = got[off:off + len(rows) * cap].reshape(len(rows), cap)
    assert np.all(got[:off] == CANARY) and np.all(got[off + len(rows) * cap:] == CANARY), "wrote outside the output"
    assert np.all(body[:, w:] == CANARY), "wrote past min(ceil(n / 8), cap)"
    for r, c in enumerate(rows):
        T, yo = reference(oracle, blk, (c, n, ""), xs[r], [n], path)
        judge(f"device {path} n={n} {what} row {r}", body[r, :w], T, yo, path, cut=w if w < nd else None,
              nch=len(rows), ncu=gpu_lib.device_cus())


# ------------------------------------------------------------------------ channels ==
def test_channels(gpu_lib, oracle):
    """3 channels at f_off 1.5 MHz, -2.2 MHz and 0 with max_segments = 6 (two segments per
    channel): each row per sample against its own truth, and bit-equal to a single-channel
    handle at the same f_off with max_segments = 2 (a wave's work depends on channel-local
    quantities only)."""
    xs = [W.stream(oracle, wbfm_input, "default", N, f_off=fo, tag=f"-ch{c}") for c, fo in enumerate(W.CH_OFFS)]
    blk = gpu_lib.WbfmChain(f_off=list(W.CH_OFFS)).configure("segmented", 6)
    got = blk.process(np.stack(xs))
    for c, fo in enumerate(W.CH_OFFS):
        one = gpu_lib.WbfmChain(f_off=fo).configure("segmented", 2)
        T, yo = reference(oracle, one, ("default", N, f"-ch{c}"), xs[c], [N], "segmented", f_off=fo)
        judge(f"channels row {c} f_off={fo:g}", got[c], T, yo, "segmented", nch=3, max_segments=6)
        single = one.process(xs[c])
        assert np.array_equal(single.view(np.uint32), got[c].view(np.uint32)), f"row {c} differs from a single-channel handle"


# ---------------------------------------------------------------------------- seek ==
@pytest.mark.parametrize("path", ["segmented", "split", "graph"])
def test_seek_across_the_oscillator_cycle(gpu_lib, oracle, path):
    """seek(2^24 - 4096 + 3): the call straddles the reference oscillator's 2^24 cycle; the
    truth takes its phasors from the oracle's Rotator run over a zero prefix."""
    n, k0 = W.SEEK_N, W.SEEK_K0
    x = W.stream(oracle, wbfm_input, "default", n, tag="-seek")
    blk = gpu_lib.WbfmChain().seek(k0).configure(path)
    T, yo = reference(oracle, blk, ("default", n, "-seek"), x, [n], path, k0=k0)
    judge(f"seek {path}", blk.process(x), T, yo, path, ncu=gpu_lib.device_cus())


# --------------------------------------------------------------------- determinism ==
@pytest.mark.parametrize("path", ["segmented", "split", "graph"])
def test_reset_and_rerun_bits(gpu_lib, oracle, path):
    """reset, then the same calls again: bit-equal output."""
    x = W.stream(oracle, wbfm_input, "default", N)
    blk = make(gpu_lib, path, 2 if path == "segmented" else 0)
    lens = W.ragged(N)
    a = run_calls(blk, x, lens)
    blk.reset()
    b = run_calls(blk, x, lens)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
