"""TEST INFRASTRUCTURE: the envelope engine of csrc/k_agc.hip (AgcRms, AgcRmsIq, CwKeyedMod)
seen from the reference alone. Validated in tests/test_agc_ref.py, used by
tests/test_gpu_agc_exact.py to prove which kernel a case reaches and which fixer it needs.

* dispatch   EnvelopeRunner restated: warmup_len (amax^W < 1e-9), chunk_len, path_of
             ('seq' k_agc_seq, 'wave' k_agc_wave, 'lane' k_agc);
* step       the switched one-pole env <- a env + (1 - a) d in numpy f32, the reference's ops
             in its order (agc.rs:33-41 with d = |x|^2 and up = d > env; cw.rs:58-62 with
             d = clamp(x, 0, 1) and up = d >= env): env_seq walks one stream in order,
             lanes_walk walks one position per chunk side by side;
* predictor  what pass 1 records for chunk c against the truth. AGC: the recorded entry is the
             end envelope of a fresh oracle.agc over x[cL - W : cL] (a fresh run seeds with
             max(d0, 1e-12), as the warm-up does), the recorded exit the same run continued to
             the chunk's end; the truth is env_seq over the whole call. CW: two trajectories
             from 0 and from 1 over the warm-up; a chunk is undetermined when they have not
             met by cL. From these: the chunks whose entry is wrong ('bad'), the ones pass 2
             flags (entry != the predecessor's recorded exit: k_agc_fix_runs re-walks them) and
             the wrong ones it does not flag ('late': only the one-wave pass 3, k_agc_fix, can
             reach them, after the run fixer changed their predecessor's exit);
* builders   seeded inputs: noise with level steps, DC / tone plateaus, CW keying, one inf.
"""
import hashlib
import math
from types import SimpleNamespace

import numpy as np

import np_ref as NR

f32 = np.float32
K_WAVE_CHUNKS = 4096   # k_agc.hip EnvelopeRunner::kWaveChunks: up to this many chunks, a wave per chunk
L_MIN = 256            # chunk_len's floor
FORGET = 1e-9          # amax^W < 1e-9
PIPE = 1 << 21         # blocks.cpp: host calls of this many samples or more are cut (2 kPipeSamples)
PIN_BYTES = 8 << 20    # ... into device calls of kPinBytes / max(in, out sample size) samples


# --------------------------------------------------------------------------- dispatch ==
def warmup_len(amax):
    """EnvelopeRunner's constructor: ceil(log(1e-9) / log(amax)) in double on the f32
    coefficient; -1 when amax >= 1 (never forgets: one sequential wave)."""
    a = float(f32(amax))
    if not a < 1.0:
        return -1
    if a <= 0.0:
        return 0
    return int(math.ceil(math.log(FORGET) / math.log(a)))


def chunk_len(n, W):
    if W < 0 or W >= n // 4:
        return n
    return max(L_MIN, (W + 15) // 16)


def n_chunks(n, W):
    L = chunk_len(n, W)
    return (n + L - 1) // L


def path_of(n, W):
    c = n_chunks(n, W)
    return "seq" if c == 1 else ("wave" if c <= K_WAVE_CHUNKS else "lane")


def host_cut(n, sample_bytes):
    """Block::host_chunked: the device calls process() makes of an n-sample host array
    (sample_bytes: the larger of the input and output sample)."""
    if n < PIPE:
        return [n]
    q = PIN_BYTES // sample_bytes
    return [min(q, n - o) for o in range(0, n, q)]


# ----------------------------------------------------------------------- coefficients ==
def agc_coefs(fs, attack_ms, release_ms):
    """agc.rs:21: a(ms) = exp(-1 / (fs * (max(ms, 1e-3) / 1000))) in f32 -> (attack_a, release_a)."""
    def a(ms):
        return NR.expf(f32(-1.0) / (f32(fs) * (max(f32(ms), f32(1e-3)) / f32(1000.0))))
    return a(attack_ms), a(release_ms)


def cw_coefs(fs, rise_ms, fall_ms):
    """cw.rs:27-30: tau = (max(ms, 0.1) 1e-3) fs, alpha = exp(-1 / tau) in f32 -> (rise, fall)."""
    def a(ms):
        return NR.expf(f32(-1.0) / ((max(f32(ms), f32(0.1)) * f32(1e-3)) * f32(fs)))
    return a(rise_ms), a(fall_ms)


def coefs(kind, cfg):
    """kind 'agc' / 'agc_iq': cfg = (fs, attack_ms, release_ms, target); 'cw': (fs, tone, rise_ms, fall_ms)."""
    return cw_coefs(cfg[0], cfg[2], cfg[3]) if kind == "cw" else agc_coefs(cfg[0], cfg[1], cfg[2])


def warm_of(kind, cfg):
    return warmup_len(max(coefs(kind, cfg)))


# ------------------------------------------------------------------------------- step ==
def drive(kind, x):
    """The recurrence's f32 input: |x|^2 (agc.rs:37 / :112, products rounded, then the sum)
    or f32::clamp(x, 0, 1) (cw.rs:56)."""
    if kind == "cw":
        x = np.asarray(x, f32)
        return np.where(x < 0, f32(0), np.where(x > 1, f32(1), x)).astype(f32)
    if kind == "agc_iq":
        x = np.asarray(x, np.complex64)
        re, im = x.real.astype(f32), x.imag.astype(f32)
        with np.errstate(over="ignore", invalid="ignore"):
            return (re * re + im * im).astype(f32)
    x = np.asarray(x, f32)
    with np.errstate(over="ignore"):
        return (x * x).astype(f32)


def env_seq(d, att, rel, env0, ge):
    """The envelope after every sample of d, in order from env0: numpy f32 scalars, one
    rounding per operation. ge: up = d >= env (CW), else d > env (AGC)."""
    att, rel = f32(att), f32(rel)
    d = np.asarray(d, f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        pa = (f32(1.0) - att) * d
        pr = (f32(1.0) - rel) * d
        out = np.empty(len(d), f32)
        e = f32(env0)
        if ge:
            for i, (dv, a, r) in enumerate(zip(d, pa, pr)):
                e = att * e + a if dv >= e else rel * e + r
                out[i] = e
        else:
            for i, (dv, a, r) in enumerate(zip(d, pa, pr)):
                e = att * e + a if dv > e else rel * e + r
                out[i] = e
    return out


def lanes_walk(d, pos, end, env, att, rel, ge, steps):
    """One trajectory per lane, side by side: lane k walks d[pos[k] : end[k]] (at most
    `steps` samples) from env[k]. Returns the envelopes (lanes past their end hold)."""
    att, rel = f32(att), f32(rel)
    oma, omr = f32(1.0) - att, f32(1.0) - rel
    pos = np.asarray(pos, np.int64).copy()
    end = np.asarray(end, np.int64)
    env = np.asarray(env, f32).copy()
    last = len(d) - 1
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for _ in range(steps):
            live = pos < end
            if not live.any():
                break
            dv = d[np.minimum(pos, last)]
            up = dv >= env if ge else dv > env
            ne = np.where(up, att * env + oma * dv, rel * env + omr * dv)
            env = np.where(live, ne, env).astype(f32)
            pos += 1
    return env


def cw_env(x, cfg, env0=0.0):
    """CwKeyedMod's envelope after every sample (cw.rs:56-62), gain 1."""
    rise, fall = cw_coefs(cfg[0], cfg[2], cfg[3])
    return env_seq(drive("cw", x), rise, fall, env0, True)


def agc_env(x, cfg, iq):
    """AgcRms / AgcRmsIq's envelope after every sample of one fresh call (seed agc.rs:57-60)."""
    kind = "agc_iq" if iq else "agc"
    d = drive(kind, x)
    att, rel = agc_coefs(cfg[0], cfg[1], cfg[2])
    return env_seq(d, att, rel, max(d[0], f32(1e-12)), False)


# -------------------------------------------------------------------------- predictor ==
def bits(a):
    return np.asarray(a, f32).view(np.uint32)


_CACHE = {}


def predict(x, cfg, kind, oracle=None):
    """Pass 1's records of one fresh call over x against the truth (module docstring).
    Returns a namespace: W, L, chunks, path, true_ent, ent, ext (NaN: undetermined), and the
    chunk lists bad, undetermined, flagged, late."""
    x = np.ascontiguousarray(x)
    key = (kind, tuple(cfg), x.dtype.str, len(x), hashlib.sha1(x.tobytes()).hexdigest())
    if key in _CACHE:
        return _CACHE[key]
    n = len(x)
    att, rel = coefs(kind, cfg)
    W = warmup_len(max(att, rel))
    L = chunk_len(n, W)
    chunks = (n + L - 1) // L
    d = drive(kind, x)
    cw = kind == "cw"
    env0 = f32(0.0) if cw else max(d[0], f32(1e-12))
    E = env_seq(d, att, rel, env0, cw)
    starts = np.arange(chunks, dtype=np.int64) * L
    ends = np.minimum(starts + L, n)
    true_ent = np.concatenate([[env0], E[starts[1:] - 1]]).astype(f32)
    true_ext = E[ends - 1]
    ent, ext = true_ent.copy(), true_ext.copy()   # chunks with cL <= W start from the carried state
    und = np.zeros(chunks, bool)
    far = np.nonzero(starts > W)[0]               # warm-up from cL - W > 0
    if len(far):
        s0 = starts[far] - W
        if cw:
            lo = lanes_walk(d, s0, starts[far], np.zeros(len(far), f32), att, rel, True, W)
            hi = lanes_walk(d, s0, starts[far], np.ones(len(far), f32), att, rel, True, W)
            und[far] = bits(lo) != bits(hi)
            ent[far] = lo
            ext[far] = lanes_walk(d, starts[far], ends[far], lo, att, rel, True, L)
            ent[und] = np.nan
            ext[und] = np.nan
        else:
            for c, a in zip(far, s0):
                ent[c] = oracle.agc(x[a:starts[c]], *cfg)[1]
                ext[c] = oracle.agc(x[a:ends[c]], *cfg)[1]
    wrong = und | (bits(ent) != bits(true_ent))
    flag = np.zeros(chunks, bool)
    flag[1:] = und[1:] | und[:-1] | (bits(ent[1:]) != bits(ext[:-1]))
    res = SimpleNamespace(
        W=W, L=L, chunks=chunks, path=path_of(n, W), true_ent=true_ent, ent=ent, ext=ext,
        bad=np.nonzero(wrong)[0].tolist(), undetermined=np.nonzero(und)[0].tolist(),
        flagged=np.nonzero(flag)[0].tolist(), late=np.nonzero(wrong & ~flag)[0].tolist())
    _CACHE[key] = res
    return res


def predict_bad(x, cfg, kind, oracle=None):
    """The chunks of one fresh call whose recorded entry differs bitwise from the truth (CW:
    the undetermined ones; a determined CW chunk is never wrong)."""
    return predict(x, cfg, kind, oracle).bad


# --------------------------------------------------------------------- input builders ==
def _cast(re, im, iq):
    return (re + 1j * im).astype(np.complex64) if iq else re.astype(f32)


def noise_steps(n, iq, seed, seg=4096):
    """Gaussian noise whose level steps every seg samples (attack and release both at work)."""
    r = np.random.default_rng(seed)
    lv = np.repeat(r.uniform(0.01, 1.5, n // seg + 1), seg)[:n]
    return _cast(lv * r.standard_normal(n), lv * r.standard_normal(n), iq)


def plateaus(n, iq, fs, seed, seg):
    """DC (real) or a pure tone (IQ) on level plateaus of seg samples with drops and rises: d
    is (nearly) constant on each, so the rounded map has a band of fixed points."""
    r = np.random.default_rng(seed)
    base = np.array([1.0, 0.5, 0.5, 0.8, 0.02, 0.02, 1.2, 0.3])
    reps = n // (seg * len(base)) + 1
    lv = np.repeat(np.tile(base, reps) * r.uniform(0.9, 1.1, reps * len(base)), seg)[:n]
    if iq:
        ph = 2 * np.pi * (1e3 / fs) * np.arange(n)
        return _cast(lv * np.cos(ph), lv * np.sin(ph), True)
    return _cast(lv, lv, False)


def with_inf(x, at):
    """x with one +inf sample (its real part) at index `at`."""
    y = np.array(x, copy=True)
    y[at] = np.inf
    return y


def cw_ragged(n, seed, dot=1000):
    """Ragged keying: on / off / partial levels and values outside [0, 1], with noise on
    every third sample (no key-up longer than `dot` samples)."""
    r = np.random.default_rng(seed)
    k = np.repeat(np.tile(np.array([1.0, 0.0, 0.6, 1.4, -0.2, 1.0, 0.0]), n // (7 * dot) + 1), dot)[:n]
    return (k + 0.01 * r.standard_normal(n) * (np.arange(n) % 3 == 0)).astype(f32)


def cw_long_keyups(n, seed, up, down):
    """Key-up stretches of about `up` samples (longer than W + L: the warm-up from 0 stalls
    below the one from 1, which stays at 1) separated by key-downs of about `down`."""
    r = np.random.default_rng(seed)
    k = np.zeros(n, f32)
    i = int(r.integers(1, down))
    while i < n:
        u = int(up * r.uniform(1.0, 1.5))
        k[i:i + u] = 1.0
        i += u + int(down * r.uniform(0.5, 1.5))
    return k


def subnormal_run(y):
    """The longest stretch of a CwKeyedMod output whose samples are nonzero and subnormal."""
    y = np.asarray(y, np.complex64)
    v = np.maximum(np.abs(y.real), np.abs(y.imag))
    m = np.concatenate([[False], (v > 0) & (v < 2.0 ** -126), [False]])
    edge = np.flatnonzero(m[1:] != m[:-1])
    return int((edge[1::2] - edge[::2]).max()) if len(edge) else 0


def cw_fall_to_subnormal(n, up_at, up_len):
    """Key-up of up_len samples at up_at, then zeros to the end of the stream."""
    k = np.zeros(n, f32)
    k[up_at:up_at + up_len] = 1.0
    return k


# ------------------------------------------------------------------------- case table ==
# (fs, attack_ms, release_ms, target) / (fs, tone_hz, rise_ms, fall_ms), with W and L
AGC = (48e3, 0.2, 4.0, 0.2)           # W 3979, L 256
AGC_BENCH = (48e3, 0.2, 5.0, 0.2)     # W 4974, L 311: tools/agc_bench.py's first case
AGC_SHORT = (48e3, 0.01, 0.01, 0.2)   # W 10: two chunks at n = 257; the envelope decays to exactly 0 on silence
CW = (48e3, 700.0, 2.0, 4.0)          # W 3979, L 256
CW_FAST = (48e3, 700.0, 0.1, 0.1)     # W 100, rise == fall: the one-coefficient walks
CW_SAME = (48e3, 700.0, 2.0, 2.0)     # W 1990, rise == fall
CW_SUB = (48e3, 700.0, 2.0, 0.1)      # W 1990: a 0.1 ms fall reaches the subnormal plateau in ~500 samples
CW_SHORT = (8e3, 700.0, 0.1, 0.2)     # W 34: two chunks at n = 257
N_LANE_RAGGED = 4097 * 256 - 37       # 4097 chunks, the last of 219 samples
N_LANE = 4098 * 256
N_LANE_BENCH = 4096 * 311 + 5         # 4097 chunks of 311, the last of 5 samples
N_WAVE_MAX = 4096 * 256               # kWaveChunks chunks exactly
N_WAVE = 64 * 256 + 1                 # 65 chunks, the last of 1 sample
N_SEQ = (1, 63, 64, 65, 257)          # one block and around it, W >= n / 4
SUB_ZEROS = 1 << 14


def kind_of(iq):
    return "agc_iq" if iq else "agc"


def cases():
    """Every single-call case of tests/test_gpu_agc_exact.py: name, kind, cfg, n, make() -> x,
    the path it must reach, and what the predictor must report: fix 'none' (no chunk bad),
    'runs' (pass 2 flags chunks: k_agc_fix_runs re-walks them) or 'both' (and wrong chunks
    it does not flag: k_agc_fix re-walks them)."""
    out = []

    def add(name, kind, cfg, n, make, path, fix):
        out.append(SimpleNamespace(name=name, kind=kind, cfg=cfg, n=n, make=make, path=path, fix=fix))

    for iq in (False, True):
        k, t = kind_of(iq), "iq" if iq else "re"
        add(f"agc-{t}-lane-noise-ragged", k, AGC, N_LANE_RAGGED, lambda iq=iq: noise_steps(N_LANE_RAGGED, iq, 3), "lane", "none")
        add(f"agc-{t}-lane-noise", k, AGC, N_LANE, lambda iq=iq: noise_steps(N_LANE, iq, 13), "lane", "none")
        add(f"agc-{t}-lane-plateaus", k, AGC, N_LANE, lambda iq=iq: plateaus(N_LANE, iq, 48e3, 4, 40_000), "lane", "both")
        add(f"agc-{t}-lane-inf", k, AGC, N_LANE_RAGGED,
            lambda iq=iq: with_inf(noise_steps(N_LANE_RAGGED, iq, 5), 3 * 256 + 7), "lane", "both")
        add(f"agc-{t}-lane-inf-last", k, AGC, N_LANE_RAGGED,   # only the last chunk's warm-up misses the inf
            lambda iq=iq: with_inf(noise_steps(N_LANE_RAGGED, iq, 22), 4096 * 256 - 3979 - 100), "lane", "runs")
        add(f"agc-{t}-lane-bench-noise", k, AGC_BENCH, N_LANE_BENCH, lambda iq=iq: noise_steps(N_LANE_BENCH, iq, 6), "lane", "none")
        add(f"agc-{t}-wave-noise-last1", k, AGC, N_WAVE, lambda iq=iq: noise_steps(N_WAVE, iq, 7), "wave", "none")
        add(f"agc-{t}-wave-plateaus-last1", k, AGC, N_WAVE, lambda iq=iq: plateaus(N_WAVE, iq, 48e3, 8, 5000), "wave", "both")
        add(f"agc-{t}-wave-plateaus-4096", k, AGC, N_WAVE_MAX, lambda iq=iq: plateaus(N_WAVE_MAX, iq, 48e3, 4, 40_000), "wave", "both")
        add(f"agc-{t}-wave-inf", k, AGC, N_WAVE, lambda iq=iq: with_inf(noise_steps(N_WAVE, iq, 9), 3 * 256 + 7), "wave", "both")
        add(f"agc-{t}-wave-inf-last", k, AGC, N_WAVE, lambda iq=iq: with_inf(noise_steps(N_WAVE, iq, 23), 64 * 256 - 3979 - 100),
            "wave", "runs")
        add(f"agc-{t}-wave-2chunks", k, AGC_SHORT, 257, lambda iq=iq: noise_steps(257, iq, 10, seg=64), "wave", "none")
        for n in N_SEQ:
            add(f"agc-{t}-seq-{n}", k, AGC, n, lambda iq=iq, n=n: noise_steps(n, iq, 11, seg=16), "seq", "none")
    add("cw-lane-ragged", "cw", CW, N_LANE_RAGGED, lambda: cw_ragged(N_LANE_RAGGED, 8), "lane", "none")
    add("cw-lane-keyups", "cw", CW, N_LANE, lambda: cw_long_keyups(N_LANE, 9, 6000, 30_000), "lane", "runs")
    add("cw-lane-fast-ragged", "cw", CW_FAST, N_LANE_RAGGED, lambda: cw_ragged(N_LANE_RAGGED, 12), "lane", "runs")
    add("cw-lane-same-ragged", "cw", CW_SAME, N_LANE_RAGGED, lambda: cw_ragged(N_LANE_RAGGED, 13), "lane", "runs")
    add("cw-lane-same-keyups", "cw", CW_SAME, N_LANE, lambda: cw_long_keyups(N_LANE, 14, 4000, 9000), "lane", "runs")
    add("cw-lane-subnormal", "cw", CW_SUB, N_LANE_RAGGED, lambda: cw_long_keyups(N_LANE_RAGGED, 15, 3000, 2 * SUB_ZEROS + 2000), "lane", "runs")
    add("cw-wave-ragged-last1", "cw", CW, N_WAVE, lambda: cw_ragged(N_WAVE, 16), "wave", "none")
    add("cw-wave-keyups-4096", "cw", CW, N_WAVE_MAX, lambda: cw_long_keyups(N_WAVE_MAX, 17, 6000, 30_000), "wave", "runs")
    add("cw-wave-fast-keyups-last1", "cw", CW_FAST, N_WAVE, lambda: cw_long_keyups(N_WAVE, 18, 500, 700), "wave", "runs")
    add("cw-wave-same-keyups-last1", "cw", CW_SAME, N_WAVE, lambda: cw_long_keyups(N_WAVE, 19, 3000, 2000), "wave", "runs")
    add("cw-wave-subnormal", "cw", CW_SUB, 3 * SUB_ZEROS, lambda: cw_fall_to_subnormal(3 * SUB_ZEROS, 5000, 3000), "wave", "runs")
    add("cw-wave-2chunks", "cw", CW_SHORT, 257, lambda: cw_ragged(257, 20, dot=40), "wave", "none")
    for n in N_SEQ:
        add(f"cw-seq-{n}", "cw", CW, n, lambda n=n: cw_ragged(n, 21, dot=20), "seq", "none")
    return out


CASES = cases()
