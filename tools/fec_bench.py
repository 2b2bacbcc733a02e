"""Times the batched soft Viterbi decode and the batched encoder of the inner code
(csrc/k_fec.hip) on device-resident data. The workload is the reference's own conv benchmark
(tests/performance/throughput/fec.rs:179-233): 512 information bits per frame, LLRs of +-4
from the coded bits, all five rates, here for both mother codes and with --frames frames
(default 4096, each with its own payload) per launch, and a single frame per launch beside
it. Counted in information bits per second. One JSON line per case, appended to --out
(default profiles/fec_bench.jsonl).

Per launch: device events around one orion_fec_viterbi_device / orion_fec_conv_encode_batch_device
call, after warm-up; median and min over --reps launches. Beside each, the library's own
host scalar decoder (orion_fec_viterbi_host, one thread of the GPU box's host, wall clock,
through ctypes) on the same input (at most --host-frames frames), and whether its bits are
the device's."""
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

INFO_BITS = 512


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


def run(code, rate, frames, warmup, reps, host_frames, out):
    L = orion_sdr._L
    c, r = orion_sdr.FEC_CODES[code], orion_sdr.FEC_RATES[rate]
    info = np.random.default_rng([0xC0DE, c, r]).integers(0, 2, (frames, INFO_BITS)).astype(np.uint8)
    d_info = torch.from_numpy(info).cuda()
    s = torch.cuda.current_stream().cuda_stream
    n_llr = orion_sdr.punctured_coded_len(INFO_BITS, rate, code)
    d_coded = torch.empty((frames, n_llr), dtype=torch.uint8, device="cuda")

    def enc():
        orion_sdr._check(L.orion_fec_conv_encode_batch_device(c, r, d_info.data_ptr(), frames, INFO_BITS, 0, 0,
                                                              d_coded.data_ptr(), s))

    emed, elo = timed(enc, warmup, reps)
    d_llr = (4.0 - 8.0 * d_coded.float()).contiguous()  # bits_to_llrs(coded, 4.0)
    d_bits = torch.empty((frames, INFO_BITS), dtype=torch.uint8, device="cuda")
    wb = int(L.orion_fec_viterbi_work_bytes(c, frames, INFO_BITS))
    work = torch.empty(wb // 8, dtype=torch.int64, device="cuda")

    def dec():
        orion_sdr._check(L.orion_fec_viterbi_device(c, r, d_llr.data_ptr(), frames, n_llr, INFO_BITS, 0, 0,
                                                    d_bits.data_ptr(), work.data_ptr(), wb, s))

    med, lo = timed(dec, warmup, reps)
    got = d_bits.cpu().numpy()
    llr = d_llr.cpu().numpy()
    nh = min(frames, host_frames)
    hbits = np.zeros(INFO_BITS, np.uint8)
    same = True
    t0 = time.perf_counter()
    for k in range(nh):
        orion_sdr._check(L.orion_fec_viterbi_host(c, r, llr[k].ctypes.data, n_llr, INFO_BITS, 0, 0, hbits.ctypes.data))
        same = same and hbits.tobytes() == got[k].tobytes()
    dt = time.perf_counter() - t0
    rec = {"case": "conv_viterbi", "code": code, "rate": rate, "info_bits": INFO_BITS, "frames": frames, "reps": reps,
           "decode_ms_median": round(med, 4), "decode_ms_min": round(lo, 4),
           "decode_info_bits_per_s": float(f"{frames * INFO_BITS / (med * 1e-3):.4g}"),
           "encode_ms_median": round(emed, 4), "encode_ms_min": round(elo, 4),
           "encode_info_bits_per_s": float(f"{frames * INFO_BITS / (emed * 1e-3):.4g}"),
           "payload_recovered": bool(np.array_equal(got, info)),
           "host_frames": nh, "host_ms": round(dt * 1e3, 3),
           "host_info_bits_per_s": float(f"{nh * INFO_BITS / dt:.4g}"), "host_equals_device": bool(same)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fec_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[4096, 1])
    ap.add_argument("--host-frames", type=int, default=256)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("fec_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for frames in a.frames:
            for code in orion_sdr.FEC_CODES:
                for rate in orion_sdr.FEC_RATES:
                    run(code, rate, frames, a.warmup, a.reps, a.host_frames, out)
