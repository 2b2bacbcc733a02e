"""Times OFDM burst acquisition and the burst receiver on device-resident captures:
ofdm_sync_batch and OfdmBurstDemod.receive_frames at --captures (default 1, 256, 4096) captures
per call, each one 2584-sample frame (n_fft 64, cp 8, 62 data carriers, QPSK, 96 payload bytes
under LDPC(n512r12) + BCH(t = 8), preamble 2 x 32 with a training symbol) after 512 samples of
lead-in, at a carrier offset spread over +-40 kHz, a random carrier phase and noise of --sigma
per part. One JSON line per case, appended to --out (default profiles/acquire_bench.jsonl).

Per case: device events around --iters back-to-back calls, after a warm-up of the same shape;
median and min of the per-call time over --reps such windows. Beside each figure: the stages of
receive_frames timed alone the same way on the tensors the stage before made (the batched search;
the carrier correction; the equalizer weights; the header's raw demodulation; its equalizer and
phase tracker), one host thread of the library's own ofdm_sync and OfdmBurstDemod.receive (wall
clock, at most --host-captures captures), and whether the device reports what the host does.
receive_frames includes its device-to-host copies of the header fields and the host-side
grouping. Nothing is asserted about speed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orion-sdr_amd"))
import orion_sdr as O  # noqa: E402

PAYLOAD, LEAD_IN, FS = 96, 512, 1e6
DATA62 = np.array([i for i in range(-31, 32) if i != 0], np.int32)


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


def us(ms):
    return round(ms * 1e3, 3)


def captures(mod, ncap, sigma):
    rng = np.random.default_rng([0xAC9, ncap])
    pay = rng.integers(0, 256, (ncap, PAYLOAD), dtype=np.uint8)
    n = LEAD_IN + mod.frame_len(1, PAYLOAD)
    x = np.zeros((ncap, n), np.complex128)
    k = np.arange(n - LEAD_IN)
    frames = mod.modulate_frames(pay, 1, sequence_nums=np.arange(ncap, dtype=np.int64))  # the batched modulator
    for c in range(ncap):
        cfo = -40e3 + 80e3 * (c + 0.5) / ncap
        x[c, LEAD_IN:] = frames[c] * np.exp(1j * (2 * np.pi * cfo * k / FS + rng.uniform(0, 2 * np.pi)))
    x += (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * sigma
    return pay, x.astype(np.complex64)


def run(ncap, a, out):
    cfg = O.OfdmConfig(64, 8, DATA62, np.zeros(0, np.int32), np.zeros(0, np.complex64), FS, 0.0, 1.0, "qpsk")
    table, pre = O.McsTable.default_ladder(), O.OfdmPreamble(2, 32).with_training_symbol(64, 8)
    mod, bd = O.OfdmFrameMod(cfg, table, pre), O.OfdmBurstDemod(cfg, table, pre)
    pay, x = captures(mod, ncap, a.sigma)
    n = x.shape[1]
    nh = min(ncap, a.host_captures)
    t0 = time.perf_counter()
    h_sync = [O.earliest_accepted(O.ofdm_sync(x[c], FS, pre, 0, n), 0.5, pre.total_len) for c in range(nh)]
    h_sync_s = (time.perf_counter() - t0) / nh
    t0 = time.perf_counter()
    h_rx = [bd.receive(x[c]) for c in range(nh)]
    h_rx_s = (time.perf_counter() - t0) / nh
    d_x = torch.from_numpy(x).cuda()
    res = {}

    def sync():
        res["s"] = O.ofdm_sync_batch(d_x, FS, pre, 0, n)

    s_med, s_min = timed(sync, a.warmup, a.reps, a.iters)

    def rx():
        res["r"] = bd.receive_frames(d_x)

    r_med, r_min = timed(rx, a.warmup, a.reps, a.iters)
    # the stages of receive_frames, each alone
    s = res["s"]
    pc = O._preamble_c(pre)
    h = O._acquire_handle(pc)
    rows = torch.empty((ncap, n), dtype=torch.complex64, device="cuda")
    avail = torch.empty(ncap, dtype=torch.int32, device="cuda")
    total = torch.empty(ncap, dtype=torch.float32, device="cuda")
    weights = torch.empty((ncap, 64), dtype=torch.complex64, device="cuda")
    oc = O._SyncOutC(**{k: s["accepted_integer_cfo_bins" if k == "accepted_bins" else k].data_ptr() for k, _, _ in O._SYNC_BATCH_KEYS})
    st = torch.cuda.current_stream().cuda_stream

    def correct():
        O._arg_check(O._L.orion_ofdm_acquire_correct_device(h, d_x.data_ptr(), ncap, n, FS, 64, C.byref(oc), rows.data_ptr(),
                                                            avail.data_ptr(), total.data_ptr(), st))

    def wts():
        O._arg_check(O._L.orion_ofdm_acquire_weights_device(h, rows.data_ptr(), ncap, n, 8, weights.data_ptr(), st))

    launches = {"sync_batch_us": us(s_med), "correct_us": us(timed(correct, a.warmup, a.reps, a.iters)[0]),
                "weights_us": us(timed(wts, a.warmup, a.reps, a.iters)[0])}
    hl = bd.header_symbols * bd.sps
    hdr = rows[:, pre.total_len:pre.total_len + hl].contiguous()
    dem = bd.demod("bpsk")

    def raw():
        res["raw"] = O.ofdm_demodulate_batch(dem, hdr, bits=False, llr=False)[0]

    launches["header_demod_raw_us"] = us(timed(raw, a.warmup, a.reps, a.iters)[0])

    def track():
        res["trk"] = dem.equalize_track(res["raw"], weights, bd.header_symbols)

    launches["header_equalize_track_us"] = us(timed(track, a.warmup, a.reps, a.iters)[0])
    g, r = {k: v.cpu().numpy() for k, v in s.items()}, res["r"]
    same_sync = all((b is None and g["accepted_start"][c] == -1) or
                    (b is not None and g["accepted_start"][c] == b.start_sample and g["accepted_integer_cfo_bins"][c] == b.integer_cfo_bins)
                    for c, b in enumerate(h_sync))
    same_rx = all((q is None and r["status"][c] == -1) or
                  (q is not None and r["status"][c] == (q.error.code if q.error else 0) and r["consume_to"][c] == q.consume_to and
                   (q.error is not None or np.array_equal(r["payloads"][c], q.packet.payload)))
                  for c, q in enumerate(h_rx))
    ok = sum(int(r["status"][c] == 0 and np.array_equal(r["payloads"][c], pay[c])) for c in range(ncap))
    nd = int(g["p"].shape[1])
    terms = (pre.num_repeats - 1) * pre.repeat_len
    rec = {"case": "acquire", "captures": ncap, "capture_samples": n, "offsets_per_capture": nd, "sigma": a.sigma,
           "reps": a.reps, "iters": a.iters,
           "sync_batch_us_median": us(s_med), "sync_batch_us_min": us(s_min),
           "sync_batch_captures_per_s": float(f"{ncap / (s_med * 1e-3):.4g}"),
           "sync_batch_msps": float(f"{ncap * n / (s_med * 1e-3) / 1e6:.4g}"),
           "sync_metric_gmacs_per_s_of_call": float(f"{ncap * nd * terms / (s_med * 1e-3) / 1e9:.4g}"),
           "receive_frames_us_median": us(r_med), "receive_frames_us_min": us(r_min),
           "receive_frames_captures_per_s": float(f"{ncap / (r_med * 1e-3):.4g}"),
           "receive_frames_msps": float(f"{ncap * n / (r_med * 1e-3) / 1e6:.4g}"),
           "decoded_with_the_sent_payload": ok,
           "host_captures": nh, "host_ofdm_sync_us_per_capture": round(h_sync_s * 1e6, 3),
           "host_receive_us_per_capture": round(h_rx_s * 1e6, 3),
           "host_equals_device_sync": bool(same_sync), "host_equals_device_receive": bool(same_rx),
           "stages_us": launches,
           "note": "sync_metric_gmacs_per_s_of_call counts the complex multiply-accumulates of the metric over the whole "
                   "call's time (select and the integer search included); the host figures are one thread"}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acquire_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--captures", type=int, nargs="*", default=[1, 256, 4096])
    ap.add_argument("--sigma", type=float, default=0.004)
    ap.add_argument("--host-captures", type=int, default=32)
    a = ap.parse_args()
    if O.device_count() < 1:
        raise SystemExit("acquire_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for ncap in a.captures:
            run(ncap, a, out)
