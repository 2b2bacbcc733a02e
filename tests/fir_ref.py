"""A plain float64 reference for the FIR family (test infrastructure, numpy only).

Standard form throughout: y[n] = sum_k g[k] x[n-k], real taps g, x real or complex,
samples before the first are the history (zeros when none is given). Everything is
computed directly (np.convolve or a scatter of taps), never through an FFT.

Three input classes make the f32 answer of a FIR unique or tightly bounded:

* integer: taps in [-7, 7], samples in [-15, 15]; every partial sum is an integer
  below 301 * 7 * 15 < 2^24, so any summation order, fused or not, is exact;
* impulse train: impulses >= K apart with amplitudes +-2^e; every output is one
  tap times a power of two plus exact zeros, exact for any f32 taps;
* dense random: |got - fir64| <= bound(x, g) per sample (the a-priori bound of a
  length-K f32 dot product, see bound()).
"""
import numpy as np

U32 = 2.0 ** -24  # unit roundoff of f32


# ---- tap layouts -------------------------------------------------------------------
def standard_taps(h):
    """FirLowpass / FirDecimator taps() (the reference's h, whose dot pairs h[L-1] with
    the newest sample and h[t] with x[n-1-t]) as the standard g: g[0] = h[L-1],
    g[k] = h[k-1]. FirLowpassIq.taps() is g already."""
    h = np.asarray(h, np.float32)
    return np.concatenate([h[-1:], h[:-1]])


# ---- the reference -----------------------------------------------------------------
def _conv_real(x, g):
    return np.convolve(np.asarray(x, np.float64), np.asarray(g, np.float64))[: len(x)]


def fir64(x, g, hist=None):
    """y[n] = sum_k g[k] x[n-k] in float64 (complex128 for complex x), len(x) outputs.
    hist: the samples before x[0], oldest first (any length; zeros before them)."""
    x = np.asarray(x)
    if hist is not None and len(hist):
        xx = np.concatenate([np.asarray(hist, x.dtype), x])
        return fir64(xx, g)[len(hist):]
    if np.iscomplexobj(x):
        return _conv_real(x.real, g) + 1j * _conv_real(x.imag, g)
    return _conv_real(x, g)


def split_calls(x, lens):
    """x cut into consecutive calls of the given lengths (which must sum to len(x))."""
    assert sum(lens) == x.shape[-1]
    o = np.concatenate([[0], np.cumsum(lens)])
    return [x[..., o[i]:o[i + 1]] for i in range(len(lens))]


def decim_pick(y_full, lens, m):
    """The per-call decimation of a full-rate output (decim.rs:44-76): the history
    carries across calls and the kept phase restarts at every call, so output j of a
    call is the full-rate output at that call's sample j * m."""
    return [c[..., ::m] for c in split_calls(y_full, lens)]


def decim64(calls, g, m):
    """Per-call outputs of the decimator over consecutive calls (a list of arrays)."""
    x = np.concatenate(list(calls))
    return decim_pick(fir64(x, g), [len(c) for c in calls], m)


def gamma(K):
    """gamma_K = (K + 1) u / (1 - (K + 1) u), u = 2^-24."""
    return (K + 1) * U32 / (1.0 - (K + 1) * U32)


def bound(x, g, hist=None):
    """The per-sample a-priori bound gamma_K sum_k |g[k]| |x[n-k]| on the error of a
    length-K f32 dot product in any association, fused or not (K products and K - 1
    sums: at most K roundings on any term). Complex x: the bound of the real parts in
    .real and of the imaginary parts in .imag (the taps are real, so they separate)."""
    x = np.asarray(x)
    ag = np.abs(np.asarray(g, np.float64))
    k = gamma(len(ag))
    if np.iscomplexobj(x):
        h = None if hist is None else np.asarray(hist)
        return k * (fir64(np.abs(x.real), ag, None if h is None else np.abs(h.real))
                    + 1j * fir64(np.abs(x.imag), ag, None if h is None else np.abs(h.imag)))
    return k * fir64(np.abs(x), ag, None if hist is None else np.abs(hist))


def worst_ratio(got, ref64, b):
    """max |got - ref64| / bound over samples and parts (inf where the bound is 0 and
    the error is not)."""
    got = np.asarray(got)
    parts = [(got.real, ref64.real, b.real), (got.imag, ref64.imag, b.imag)] if np.iscomplexobj(got) else [(got, ref64, b)]
    w = 0.0
    for a, r, bb in parts:
        e = np.abs(np.asarray(a, np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(e == 0.0, 0.0, e / bb)
        w = max(w, float(q.max()) if q.size else 0.0)
    return w


def same(got, ref64):
    """Exact comparison by value (+0.0 == -0.0) of got with the float64 reference
    rounded to got's f32 type; also requires every output to be finite."""
    got = np.asarray(got)
    ref = np.asarray(ref64).astype(got.dtype)
    return got.shape == ref.shape and bool(np.all(np.isfinite(got))) and np.array_equal(got, ref)


def first_diffs(got, ref64, limit=8):
    """Indices (flat) of the first mismatches, for a failure message."""
    got = np.asarray(got)
    ref = np.asarray(ref64).astype(got.dtype)
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    idx = np.flatnonzero(got.ravel() != ref.ravel())
    return f"{idx.size} differ, first at {idx[:limit].tolist()}"


# ---- input classes -----------------------------------------------------------------
def int_taps(K, seed=0):
    """Integer taps in [-7, 7], asymmetric: first, middle and last tap nonzero and
    pairwise different (so not a palindrome) once K >= 3."""
    rng = np.random.default_rng(1000 + 7 * K + seed)
    h = rng.integers(-7, 8, K).astype(np.float32)
    if K >= 3:
        h[0], h[K // 2], h[K - 1] = 3.0, -5.0, 7.0
    elif K == 2:
        h[:] = [3.0, -5.0]
    else:
        h[:] = [3.0]
    return h


def int_samples(shape, seed=0, complex_=True):
    """Integers in [-15, 15] (re and im independently)."""
    rng = np.random.default_rng(2000 + seed)
    if not complex_:
        return rng.integers(-15, 16, shape).astype(np.float32)
    return (rng.integers(-15, 16, shape) + 1j * rng.integers(-15, 16, shape)).astype(np.complex64)


def dense_samples(shape, seed=0, complex_=True):
    """Standard-normal f32 (re and im independently)."""
    rng = np.random.default_rng(3000 + seed)
    if not complex_:
        return rng.standard_normal(shape).astype(np.float32)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def impulses(n, d, first, seed=0, complex_=True):
    """An impulse train: positions first, first + d, ... below n and one amplitude
    +-2^e, e in [-3, 3], per impulse (complex: re and im chosen independently and
    made different). Returns (pos int64, amp)."""
    assert d >= 1 and first >= 0
    rng = np.random.default_rng(4000 + seed)
    pos = np.arange(first, n, d, dtype=np.int64)

    def amps():
        return rng.choice([-1.0, 1.0], len(pos)) * 2.0 ** rng.integers(-3, 4, len(pos))

    re = amps()
    if not complex_:
        return pos, re.astype(np.float32)
    im = amps()
    im = np.where(im == re, -im, im)
    return pos, (re + 1j * im).astype(np.complex64)


def impulse_signal(n, pos, amp):
    x = np.zeros(n, amp.dtype)
    x[pos] = amp
    return x


def impulse_fir64(n, pos, amp, g):
    """fir64 of impulse_signal(n, pos, amp) with zero history, as a scatter of taps:
    y[p + k] = amp g[k]. The impulses must be >= len(g) apart (no two overlap)."""
    g = np.asarray(g, np.float64)
    K = len(g)
    assert len(pos) < 2 or int(np.min(np.diff(pos))) >= K, "impulses closer than the filter is long"
    y = np.zeros(n + K, np.complex128 if np.iscomplexobj(amp) else np.float64)
    if len(pos):
        y[(pos[:, None] + np.arange(K)[None, :]).ravel()] = (amp.astype(y.dtype)[:, None] * g[None, :]).ravel()
    return y[:n]
