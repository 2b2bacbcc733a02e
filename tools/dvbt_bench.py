"""Times the batched DVB-T frame path on device-resident tensors: DvbTFrameMod.modulate_frames,
DvbTFrameDemod.decode_frames and dvb_t_gi_sync_batch alone at --frames (default 1, 16, 256) frames
of 68 symbols per call, for QPSK 1/2 guard 1/32 and 16-QAM 3/4 guard 1/8, each frame carrying the
largest payload that still fits 68 symbols, each capture the frame after 200 samples of lead-in
with noise of --noise times the frame's rms. One JSON line per case, appended to --out (default
profiles/dvbt_bench.jsonl).

Per case: device events around --iters back-to-back calls after a warm-up of the same shape, median
and min of the per-call time over --reps such windows (the calls end in their own device-to-host
copies, so the events cover them). Beside each figure: one host thread of the library's own
modulate / decode / dvb_t_gi_sync (wall clock, at most --host-frames frames), the wall-clock share
of each call spent in the host-side TS adaptation (packets, null-packet stuffing, energy dispersal
on the way in; de-dispersal and depacketizing on the way out), timed alone on the same data, and
whether the device reports what the host does. Nothing is asserted about speed."""
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
import orion_sdr as O  # noqa: E402

LEAD_IN = 200
LINKS = (("1/32", "qpsk", "1/2"), ("1/8", "qam16", "3/4"))


def timed(fn, warmup, reps, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) / iters)
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms), statistics.median(wall)


def us(ms):
    return round(ms * 1e3, 1)


def wall_of(fn, n):
    t0 = time.perf_counter()
    out = [fn(k) for k in range(n)]
    return (time.perf_counter() - t0) / max(n, 1), out


def full_payload_len(mod):
    """The most TS packets whose frame is still 68 symbols, in payload bytes."""
    lo, hi = 1, 400
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mod.plan(mid * 187)[0] <= 68:
            lo = mid
        else:
            hi = mid - 1
    return lo * 187


def run(link, frames, a, out):
    guard, con, rate = link
    p = O.DvbTFrameParams(guard, con, rate, 0, 0)
    mod, demod = O.DvbTFrameMod(p), O.DvbTFrameDemod(p)
    n = full_payload_len(mod)
    n_symbols, target = mod.plan(n)
    sps = O.DVB_T_N_FFT + p.cp_len
    rng = np.random.default_rng([0xD7B, frames])
    pay = rng.integers(0, 256, (frames, n), dtype=np.uint8)
    fn = (np.arange(frames) % 4).astype(np.int64)
    ci = (np.arange(frames) % 256).astype(np.int64)
    nh = min(frames, a.host_frames)
    iters = max(1, a.iters // max(frames // 16, 1))

    d_pay = torch.from_numpy(pay).cuda()
    iq = mod.modulate_frames(d_pay, frame_numbers=fn, cell_ids=ci)
    h_mod_s, h_iq = wall_of(lambda k: O.DvbTFrameMod(p.with_frame(int(fn[k]), int(ci[k]))).modulate(pay[k]).iq, nh)
    mod_same = all(np.array_equal(iq[k].cpu().numpy().view(np.uint32), h_iq[k].view(np.uint32)) for k in range(nh))
    m_med, m_min, m_wall = timed(lambda: mod.modulate_frames(d_pay, frame_numbers=fn, cell_ids=ci), a.warmup, a.reps, iters)
    ts_in_s, _ = wall_of(lambda k: mod._ts(pay[k % frames], target), frames)

    x = iq.cpu().numpy()
    r = float(np.sqrt(np.mean(np.abs(x[0].astype(np.complex128)) ** 2)))
    caps = np.zeros((frames, LEAD_IN + x.shape[1] + 100), np.complex64)
    caps[:, LEAD_IN:LEAD_IN + x.shape[1]] = x
    caps += ((rng.standard_normal(caps.shape) + 1j * rng.standard_normal(caps.shape)) * (a.noise * r / np.sqrt(2))).astype(np.complex64)
    d_caps = torch.from_numpy(caps).cuda()
    res = demod.decode_frames(d_caps, n_symbols, n)

    def host_decode(k):
        try:
            return demod.decode(caps[k], n_symbols, n)
        except O.DvbTRxError as e:
            return e.code

    h_dec_s, h_rx = wall_of(host_decode, nh)
    dec_same = all((res["error"][k] == h_rx[k]) if isinstance(h_rx[k], int) else
                   (res["error"][k] == 0 and np.array_equal(res["payloads"][k], h_rx[k].payload) and
                    res["timing_offset_samples"][k] == h_rx[k].diagnostics["timing_offset_samples"]) for k in range(nh))
    d_med, d_min, d_wall = timed(lambda: demod.decode_frames(d_caps, n_symbols, n), a.warmup, a.reps, iters)
    packets = max(1, -(-n // 187))
    dispersed = [mod._ts(pay[k], target)[:packets * 188] for k in range(min(frames, 16))]
    ts_out_s, _ = wall_of(lambda k: O.ts_depacketize(O.ts_energy_disperse(dispersed[k % len(dispersed)])), frames)

    s_med, s_min, _ = timed(lambda: O.dvb_t_gi_sync_batch(d_caps, O.DVB_T_N_FFT, p.cp_len, p.fs, sps), a.warmup, a.reps, iters)
    h_sync_s, h_sync = wall_of(lambda k: O.dvb_t_gi_sync(caps[k], O.DVB_T_N_FFT, p.cp_len, p.fs, sps), nh)
    starts = O.dvb_t_gi_sync_batch(d_caps, O.DVB_T_N_FFT, p.cp_len, p.fs, sps)["start"].cpu().numpy()
    sync_same = all(int(starts[k]) == h_sync[k].start_sample for k in range(nh))

    line = {
        "bench": "dvbt", "guard": guard, "constellation": con, "code_rate": rate, "frames": frames, "n_symbols": n_symbols,
        "payload_bytes": n, "ts_packets": target, "samples_per_frame": int(x.shape[1]), "noise_over_rms": a.noise,
        "iters": iters, "reps": a.reps, "decoded": int(np.count_nonzero(res["error"] == 0)),
        "modulate_frames_us": us(m_med), "modulate_frames_min_us": us(m_min), "modulate_frames_us_per_frame": us(m_med / frames),
        "modulate_host_us_per_frame": round(h_mod_s * 1e6, 1), "modulate_ts_host_share": round(ts_in_s * frames / m_wall, 3),
        "modulate_equals_host": bool(mod_same),
        "decode_frames_us": us(d_med), "decode_frames_min_us": us(d_min), "decode_frames_us_per_frame": us(d_med / frames),
        "decode_host_us_per_frame": round(h_dec_s * 1e6, 1), "decode_ts_host_share": round(ts_out_s * frames / d_wall, 3),
        "decode_equals_host": bool(dec_same),
        "gi_sync_batch_us": us(s_med), "gi_sync_batch_min_us": us(s_min), "gi_sync_batch_us_per_capture": us(s_med / frames),
        "gi_sync_host_us_per_capture": round(h_sync_s * 1e6, 1), "gi_sync_equals_host": bool(sync_same),
        "host_frames": nh, "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(line))
    out.write(json.dumps(line) + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dvbt_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dvbt_bench: no GPU visible; timings are taken on the device only")
    with open(a.out, "a") as out:
        for link in LINKS:
            for frames in a.frames:
                run(link, frames, a, out)


if __name__ == "__main__":
    main()
