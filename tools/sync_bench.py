"""Times ft8_sync / ft4_sync (sync/ft8_sync.rs, sync/ft4_sync.rs) on device-resident input:
a full FT8 slot (180,000 samples) and a full FT4 slot (90,000 samples), searched over
0 .. 3 kHz with t_min = -2, t_max = 12 and 20 candidates, at 1, 16 and 256 channels, for
every rows-per-lane form of the waterfall kernel (0 = the engine's own choice). One JSON
line per case, appended to --out (default profiles/sync_bench.jsonl).

Per launch: device events around one orion_ft*_sync_device call (waterfall + search +
LLRs), after warm-up; median and min over --reps launches. "wf_ms" times the waterfall
kernel alone the same way.

Work: a cell-sample is one complex multiply-accumulate of the waterfall (one sample into
one (row, tone) cell): nch * num_bins * (samples the rows hold). Its floor on the vector
ALU is 8 f32 lane-operations (4 multiplies, 2 adds / subtracts of the non-fused complex
product, 2 accumulating adds: 4 packed instructions); the shared phasor recurrence adds
4 / rows-per-lane. frac_pk_f32 = cell-samples/s * 8 / PK_LANE_OPS, with PK_LANE_OPS the
packed-FP32 issue rate, 157.3e12 / 2 lane-operations per second (the vector FP32 peak
counts an FMA as two). Beside them, the numpy restatement (tests/np_ref_sync.py) on one
channel, host wall clock.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orion-sdr_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orion_sdr  # noqa: E402

PK_LANE_OPS = 157.3e12 / 2
FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND = 12000.0, 0.0, 3000.0, -2, 12, 20
MODES = {"ft8": dict(n=180_000, sps=1920, spacing=6.25), "ft4": dict(n=90_000, sps=576, spacing=20.833334)}


def cell_samples(pat, nch):
    m = MODES[pat]
    num_bins, wf_syms, start, _, _ = orion_sdr.sync_geometry(pat, BASE_HZ, MAX_HZ, T_MIN, T_MAX)
    held = sum(max(0, min(m["sps"], m["n"] - (start + r * m["sps"]))) for r in range(wf_syms))
    return nch * num_bins * held, num_bins, wf_syms, start


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def run(pat, nch, rows, warmup, reps, out):
    m = MODES[pat]
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.view_as_complex(torch.randn((nch, m["n"], 2), device="cuda", generator=g))
    work, num_bins, wf_syms, start = cell_samples(pat, nch)
    eng = orion_sdr.SyncEngine().set_rows_per_lane(rows)
    L = orion_sdr._L
    cand = torch.empty((nch, MAX_CAND, 3), dtype=torch.int32, device="cuda")
    count = torch.empty((nch,), dtype=torch.int32, device="cuda")
    llr = torch.empty((nch, MAX_CAND, 174), dtype=torch.float32, device="cuda")
    wf = torch.empty((nch, wf_syms, num_bins), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    fn = L.orion_ft8_sync_device if pat == "ft8" else L.orion_ft4_sync_device

    def full():
        orion_sdr._check(fn(eng._h, x.data_ptr(), nch, m["n"], FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND,
                            cand.data_ptr(), count.data_ptr(), llr.data_ptr(), s))

    def wf_only():
        orion_sdr._check(L.orion_waterfall_compute_device(eng._h, x.data_ptr(), FS, BASE_HZ, m["spacing"], m["sps"],
                                                          wf_syms, num_bins, start, nch, m["n"], 0, wf.data_ptr(), s))

    med, lo = timed(full, warmup, reps)
    wmed, wlo = timed(wf_only, warmup, reps)
    rate = work / (wmed * 1e-3)
    rec = {"case": f"{pat}_sync", "nch": nch, "n_per_ch": m["n"], "rows_per_lane": rows, "wf_syms": wf_syms,
           "num_bins": num_bins, "reps": reps, "sync_ms_median": round(med, 4), "sync_ms_min": round(lo, 4),
           "wf_ms_median": round(wmed, 4), "wf_ms_min": round(wlo, 4), "cell_samples": work,
           "wf_cell_samples_per_s": float(f"{rate:.4g}"), "wf_frac_pk_f32": round(rate * 8 / PK_LANE_OPS, 4),
           "slots_per_s": round(nch / (med * 1e-3), 1)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def run_numpy(pat, out):
    import np_ref_sync as S

    m = MODES[pat]
    rng = np.random.default_rng(7)
    iq = (rng.standard_normal(m["n"]) + 1j * rng.standard_normal(m["n"])).astype(np.complex64)
    t0 = time.perf_counter()
    S.sync(iq, S.FT8 if pat == "ft8" else S.FT4, FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND)
    dt = time.perf_counter() - t0
    work = cell_samples(pat, 1)[0]
    rec = {"case": f"{pat}_sync numpy restatement (host, one run)", "nch": 1, "n_per_ch": m["n"],
           "sync_ms": round(dt * 1e3, 1), "cell_samples": work, "cell_samples_per_s": float(f"{work / dt:.4g}")}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--rows", type=int, nargs="*", default=[0, 1, 2, 4, 8])
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("sync_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for pat in ("ft8", "ft4"):
            for nch in a.channels:
                for rows in a.rows:
                    run(pat, nch, rows, a.warmup, max(20, a.reps), out)
            if not a.no_numpy:
                run_numpy(pat, out)
