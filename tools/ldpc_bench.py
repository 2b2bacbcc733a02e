"""Times the batched LDPC(174,91) + CRC-14 decode (csrc/k_ldpc.hip) on device-resident
LLRs: 1, 80 and 5120 codewords (5120 = 256 channels x 20 candidates, a slot of
tools/sync_bench.py) of three kinds of input,
  valid    encoded words at +-10: the initial decision is valid, no iteration runs
  sigma0.7 BPSK + noise (sigma 0.7, scaled to mean square 24) under the sum_product rule
  noise    Gaussian LLRs: every word runs all 20 iterations (the worst case)
and ft8_decode against ft8_sync alone at 1, 16 and 256 channels x 20 candidates in the same
process (what decoding adds to a slot). One JSON line per case, appended to --out (default
profiles/ldpc_bench.jsonl).

Per launch: device events around one orion_ldpc_decode_device call, after warm-up; median
and min over --reps launches. Beside each, the library's own host scalar decoder
(orion_ldpc_decode_host, one thread of the GPU box's host, wall clock, through ctypes) on
the same words (at most --host-words of them)."""
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

FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND = 12000.0, 0.0, 3000.0, -2, 12, 20
N_SLOT = 180_000


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


def words(kind, n):
    import np_ref_ldpc as R

    rng = np.random.default_rng(70)
    if kind == "noise":
        x = rng.standard_normal((n, 174))
        return (x * np.sqrt(24.0 / (x * x).mean(axis=1, keepdims=True))).astype(np.float32)
    base = []
    for _ in range(min(n, 64)):  # 64 distinct words, repeated with fresh noise
        base.append(R.codeword_bits("ft8", R.random_payload(rng)))
    out = np.empty((n, 174), np.float32)
    for k in range(n):
        bits = base[k % len(base)]
        out[k] = np.where(bits == 1, -10.0, 10.0) if kind == "valid" else R.noisy_llr(bits, 0.7, rng)
    return out


def run_decode(kind, n, rule, warmup, reps, host_words, out):
    x = words(kind, n)
    d = torch.from_numpy(x).cuda()
    res = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L = orion_sdr._L
    rl = orion_sdr._rule(rule)

    def dev():
        orion_sdr._check(L.orion_ldpc_decode_device(d.data_ptr(), n, None, 0, 0, rl, 20, res.data_ptr(), None, s))

    med, lo = timed(dev, warmup, reps)
    rec_dev = res.cpu().numpy().view(orion_sdr.RESULT_DTYPE)[:, 0]
    nh = min(n, host_words)
    hres = np.zeros(1, orion_sdr.RESULT_DTYPE)
    t0 = time.perf_counter()
    same = True
    for k in range(nh):
        orion_sdr._check(L.orion_ldpc_decode_host(x[k].ctypes.data, 0, rl, 20, hres.ctypes.data, None))
        same = same and hres[0].tobytes() == rec_dev[k].tobytes()
    dt = time.perf_counter() - t0
    rec = {"case": "ldpc_decode", "input": kind, "rule": rule, "n": n, "reps": reps,
           "ms_median": round(med, 4), "ms_min": round(lo, 4), "codewords_per_s": float(f"{n / (med * 1e-3):.4g}"),
           "decoded": int((rec_dev["status"] == 2).sum()), "mean_iterations": round(float(rec_dev["iterations"].mean()), 2),
           "host_words": nh, "host_ms": round(dt * 1e3, 3), "host_codewords_per_s": float(f"{nh / dt:.4g}"),
           "host_equals_device": bool(same)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def run_pipeline(nch, rule, warmup, reps, out):
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.view_as_complex(torch.randn((nch, N_SLOT, 2), device="cuda", generator=g))
    eng = orion_sdr.SyncEngine()
    L = orion_sdr._L
    cand = torch.empty((nch, MAX_CAND, 3), dtype=torch.int32, device="cuda")
    count = torch.empty((nch,), dtype=torch.int32, device="cuda")
    llr = torch.empty((nch, MAX_CAND, 174), dtype=torch.float32, device="cuda")
    res = torch.empty((nch, MAX_CAND, 4), dtype=torch.int32, device="cuda")
    pick = torch.empty((nch, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    geo = (nch, N_SLOT, FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND)

    def sync():
        orion_sdr._check(L.orion_ft8_sync_device(eng._h, x.data_ptr(), *geo, cand.data_ptr(), count.data_ptr(),
                                                 llr.data_ptr(), s))

    def decode():
        orion_sdr._check(L.orion_ft8_decode_device(eng._h, x.data_ptr(), *geo, orion_sdr._rule(rule), 20, cand.data_ptr(),
                                                   count.data_ptr(), llr.data_ptr(), res.data_ptr(), pick.data_ptr(), s))

    smed, slo = timed(sync, warmup, reps)
    dmed, dlo = timed(decode, warmup, reps)
    rec = {"case": "ft8_decode vs ft8_sync", "input": "noise slot (every candidate runs 20 iterations)", "rule": rule,
           "nch": nch, "max_cand": MAX_CAND, "n_per_ch": N_SLOT, "reps": reps, "sync_ms_median": round(smed, 4),
           "sync_ms_min": round(slo, 4), "decode_ms_median": round(dmed, 4), "decode_ms_min": round(dlo, 4),
           "added_ms_median": round(dmed - smed, 4), "slots_per_s": round(nch / (dmed * 1e-3), 1)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpc_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 80, 5120])
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--host-words", type=int, default=512)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("ldpc_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for kind, rule in (("valid", "reference"), ("sigma0.7", "sum_product"), ("noise", "reference")):
            for n in a.sizes:
                run_decode(kind, n, rule, a.warmup, max(20, a.reps), a.host_words, out)
        for nch in a.channels:
            run_pipeline(nch, "reference", a.warmup, max(20, a.reps), out)
