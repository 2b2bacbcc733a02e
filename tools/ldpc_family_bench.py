"""Times the frame chain's two codes on device-resident data: the batched LDPC family decode
(csrc/k_ldpc_family.hip) of --words (default 4096, and 1 beside it) codewords per launch, per
code and check rule, at a noise level where words need several iterations (BPSK plus Gaussian
noise, llr = 2 y / sigma^2; the mean iteration count per word is reported, since the time
follows it), and the batched BCH(184, 120, t = 8) decode (csrc/k_bch.hip) of as many words
with 0, 4, 8 and 9 bit errors (9 is past t: the whole decoder runs and the word is rejected).
The two encoders are timed on the same shapes. One JSON line per case, appended to --out
(default profiles/ldpc_family_bench.jsonl).

Per case: device events around --iters back-to-back launches, after a warm-up of the same
shape; median and min of the per-launch time over --reps such windows. Beside each, one host
thread of the library's own scalar code (wall clock, through ctypes) on the same words (at
most --host-words of them), and whether every output of it is the device's."""
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
import orion_sdr  # noqa: E402

SIGMA = {"n512r12": 0.7, "n576r23": 0.6, "n512r34": 0.55}
RULES = ("sum_product", "min_sum", ("scaled_min_sum", 0.75))
BCH_T, BCH_N, BCH_K = 8, 184, 120


def timed(fn, warmup, reps, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms)


def rate(count, ms):
    return float(f"{count / (ms * 1e-3):.4g}")


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def run_ldpc(code, rule, words, a, out):
    c = orion_sdr.Ldpc(code)
    rng = np.random.default_rng([0x1D9C, c.index, words])
    msgs = rng.integers(0, 2, (words, c.k), dtype=np.uint8)
    sigma = SIGMA[code]
    y = (1.0 - 2.0 * c.encode(msgs)) + sigma * rng.standard_normal((words, c.n))
    llr = (2.0 * y / sigma ** 2).astype(np.float32)
    nh = min(words, a.host_words)
    t0 = time.perf_counter()
    hb, hu, hi = c.decode_soft(llr[:nh], 50, rule)
    dt = time.perf_counter() - t0
    d_llr = torch.from_numpy(llr.reshape(1, -1)).cuda()
    res = {}

    def dec():
        res["r"] = orion_sdr.ldpc_family_decode_batch(d_llr, code, rule=rule)

    med, lo = timed(dec, a.warmup, a.reps, a.iters)
    gb, gu, gi = (t.cpu().numpy().reshape(words, -1) for t in res["r"])
    same = np.array_equal(gb[:nh], hb) and np.array_equal(gu[:nh, 0], hu) and np.array_equal(gi[:nh, 0], hi)
    emit({"case": "ldpc_family_decode", "code": code, "rule": rule if isinstance(rule, str) else list(rule),
          "words": words, "sigma": sigma, "max_iter": 50, "mean_iterations": round(float(gi.mean()), 3),
          "failed_words": int((gu > 0).sum()), "message_errors": int((gb != msgs).any(axis=1).sum()),
          "reps": a.reps, "iters": a.iters, "decode_us_median": round(med * 1e3, 3), "decode_us_min": round(lo * 1e3, 3),
          "decode_words_per_s": rate(words, med), "decode_coded_bits_per_s": rate(words * c.n, med),
          "host_words": nh, "host_us_per_word": round(dt * 1e6 / nh, 3), "host_words_per_s": float(f"{nh / dt:.4g}"),
          "host_equals_device": bool(same)}, out)


def run_ldpc_encode(code, words, a, out):
    c = orion_sdr.Ldpc(code)
    msgs = np.random.default_rng([0xE2C, c.index, words]).integers(0, 2, (words, c.k), dtype=np.uint8)
    d = torch.from_numpy(msgs.reshape(1, -1)).cuda()
    res = {}

    def enc():
        res["c"] = orion_sdr.ldpc_family_encode_batch(d, code)

    med, lo = timed(enc, a.warmup, a.reps, a.iters)
    nh = min(words, a.host_words)
    t0 = time.perf_counter()
    want = c.encode(msgs[:nh])
    dt = time.perf_counter() - t0
    emit({"case": "ldpc_family_encode", "code": code, "words": words, "reps": a.reps, "iters": a.iters,
          "encode_us_median": round(med * 1e3, 3), "encode_us_min": round(lo * 1e3, 3),
          "encode_words_per_s": rate(words, med), "host_words": nh, "host_us_per_word": round(dt * 1e6 / nh, 3),
          "host_equals_device": bool(np.array_equal(res["c"].cpu().numpy().reshape(words, c.n)[:nh], want))}, out)


def run_bch(words, n_err, a, out):
    code = orion_sdr.Bch.for_info_bits(BCH_T)
    rng = np.random.default_rng([0xBC4, words, n_err])
    msgs = rng.integers(0, 2, (words, BCH_K), dtype=np.uint8)
    rx = code.encode(msgs)
    for w in rx:
        w[rng.choice(BCH_N, n_err, replace=False)] ^= 1
    nh = min(words, a.host_words)
    t0 = time.perf_counter()
    hm, hs = code.decode_counted(rx[:nh])
    dt = time.perf_counter() - t0
    d_in = torch.from_numpy(rx.reshape(1, -1)).cuda()
    res = {}

    def dec():
        res["m"], res["s"] = orion_sdr.bch_decode_batch(d_in, BCH_T)

    med, lo = timed(dec, a.warmup, a.reps, a.iters)
    gm, gs = res["m"].cpu().numpy().reshape(words, BCH_K)[:nh], res["s"].cpu().numpy().reshape(words)[:nh]
    rec = {"case": "bch_decode", "n": BCH_N, "k": BCH_K, "t": BCH_T, "words": words, "errors_per_word": n_err,
           "reps": a.reps, "iters": a.iters, "decode_us_median": round(med * 1e3, 3), "decode_us_min": round(lo * 1e3, 3),
           "decode_words_per_s": rate(words, med), "uncorrectable": int((hs < 0).sum()), "host_words": nh,
           "host_us_per_word": round(dt * 1e6 / nh, 3), "host_words_per_s": float(f"{nh / dt:.4g}"),
           "host_equals_device": bool(np.array_equal(gs, hs) and np.array_equal(gm, hm))}
    if n_err == 0:
        d_msgs = torch.from_numpy(msgs.reshape(1, -1)).cuda()

        def enc():
            res["c"] = orion_sdr.bch_encode_batch(d_msgs, BCH_T)

        emed, elo = timed(enc, a.warmup, a.reps, a.iters)
        rec.update({"encode_us_median": round(emed * 1e3, 3), "encode_us_min": round(elo * 1e3, 3),
                    "encode_equals_host": bool(np.array_equal(res["c"].cpu().numpy().reshape(words, BCH_N), rx))})
    emit(rec, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpc_family_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--words", type=int, nargs="*", default=[4096, 1])
    ap.add_argument("--errors", type=int, nargs="*", default=[0, 4, 8, 9])
    ap.add_argument("--host-words", type=int, default=1024)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("ldpc_family_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for words in a.words:
            for code in SIGMA:
                for rule in RULES:
                    run_ldpc(code, rule, words, a, out)
                run_ldpc_encode(code, words, a, out)
            for n_err in a.errors:
                run_bch(words, n_err, a, out)
