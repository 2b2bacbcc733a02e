"""Times the batched Reed-Solomon decode of the outer code (csrc/k_rs.hip) on device-resident
data: --words (default 4096, and 1 beside it) RS(204,188) codewords per launch, each with its
own random message, with 0, 4, 8 and 9 byte errors per word (9 is past t = 8: the whole
decoder runs and the word is rejected), as plain bytes and with all three fusions (one bit per
byte in, the (12, 17) Forney deinterleaver in the fetch, energy dispersal in the store; the
words are then one stream). The batched encoder and the frame interleaver are timed on the same
shape. Counted in codewords and message bits per second. One JSON line per case, appended to
--out (default profiles/rs_bench.jsonl).

Per case: device events around --iters back-to-back launches, after a warm-up of the same
shape; median and min of the per-launch time over --reps such windows. Beside each, one host
thread of the library's own decode_counted (orion_rs_decode_counted, wall clock, through
ctypes) on the same words (at most --host-words of them), and whether its messages and status
words are the device's."""
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

N, NP, K = 204, 16, 188
IL = (12, 17)


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


def received(words, n_err):
    rng = np.random.default_rng([0x5EED, words, n_err])
    cws = orion_sdr.ReedSolomon(N, NP).encode(rng.integers(0, 256, (words, K), dtype=np.uint8))
    for cw in cws:
        pos = rng.choice(N, n_err, replace=False)
        cw[pos] ^= rng.integers(1, 256, n_err, dtype=np.uint8)
    return cws


def rate(count, ms):
    return float(f"{count / (ms * 1e-3):.4g}")


def run_decode(words, n_err, fused, a, out):
    rx = received(words, n_err)
    nh = min(words, a.host_words)
    hm, hs = np.zeros((nh, K), np.uint8), np.zeros(nh, np.int32)
    t0 = time.perf_counter()
    orion_sdr._check(orion_sdr._L.orion_rs_decode_counted(N, NP, rx.ctypes.data, nh, hm.ctypes.data, hs.ctypes.data))
    dt = time.perf_counter() - t0
    if fused:
        stream = np.unpackbits(orion_sdr.forney_frame_interleave(rx.reshape(-1), *IL))
        d_in = torch.from_numpy(stream).cuda()
        kw = dict(bits=True, deinterleave=IL, derandomize=True)
        want_m = orion_sdr.ts_energy_disperse(hm.reshape(-1)).reshape(nh, K)
    else:
        d_in = torch.from_numpy(rx).cuda()
        kw, want_m = {}, hm
    res = {}

    def dec():
        res["m"], res["s"] = orion_sdr.rs_decode_batch(d_in, **kw)

    med, lo = timed(dec, a.warmup, a.reps, a.iters)
    gm, gs = res["m"].cpu().numpy()[:nh], res["s"].cpu().numpy()[:nh]
    rec = {"case": "rs_decode", "n": N, "k": K, "words": words, "errors_per_word": n_err,
           "input": "bits+deinterleave+derandomize" if fused else "bytes", "reps": a.reps, "iters": a.iters,
           "decode_us_median": round(med * 1e3, 3), "decode_us_min": round(lo * 1e3, 3),
           "decode_words_per_s": rate(words, med), "decode_message_bits_per_s": rate(words * K * 8, med),
           "uncorrectable": int((hs < 0).sum()), "host_words": nh, "host_us_per_word": round(dt * 1e6 / nh, 3),
           "host_words_per_s": float(f"{nh / dt:.4g}"),
           "host_equals_device": bool(np.array_equal(gs, hs) and np.array_equal(gm, want_m))}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def run_encode(words, a, out):
    rng = np.random.default_rng([0xE2C, words])
    msgs = rng.integers(0, 256, (words, K), dtype=np.uint8)
    d_msgs = torch.from_numpy(msgs).cuda()
    res = {}

    def enc():
        res["c"] = orion_sdr.rs_encode_batch(d_msgs, disperse=True)

    emed, elo = timed(enc, a.warmup, a.reps, a.iters)
    d_cws = res["c"]

    def il():
        res["i"] = orion_sdr.forney_interleave_batch(d_cws.view(-1), *IL, bits=True)

    imed, ilo = timed(il, a.warmup, a.reps, a.iters)
    nh = min(words, a.host_words)
    t0 = time.perf_counter()
    want = orion_sdr.ReedSolomon(N, NP).encode(orion_sdr.ts_energy_disperse(msgs[:nh].reshape(-1)).reshape(nh, K))
    dt = time.perf_counter() - t0
    rec = {"case": "rs_encode", "n": N, "k": K, "words": words, "reps": a.reps, "iters": a.iters,
           "encode_us_median": round(emed * 1e3, 3), "encode_us_min": round(elo * 1e3, 3),
           "encode_words_per_s": rate(words, emed),
           "interleave_bits_us_median": round(imed * 1e3, 3), "interleave_bits_us_min": round(ilo * 1e3, 3),
           "host_words": nh, "host_us_per_word": round(dt * 1e6 / nh, 3),
           "host_equals_device": bool(np.array_equal(d_cws.cpu().numpy()[:nh], want))}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rs_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--words", type=int, nargs="*", default=[4096, 1])
    ap.add_argument("--errors", type=int, nargs="*", default=[0, 4, 8, 9])
    ap.add_argument("--host-words", type=int, default=4096)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("rs_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for words in a.words:
            for n_err in a.errors:
                for fused in (False, True):
                    run_decode(words, n_err, fused, a, out)
            run_encode(words, a, out)
