"""Times the FT8 modulator, the slot synthesiser and the hard demodulator (csrc/k_ftmod.hip)
on device-resident buffers, and ft8_decode on synthesised slots. One JSON line per case,
appended to --out (default profiles/ftmod_bench.jsonl).

  modulate    Ft8Mod.modulate of 1, 16 and 256 frames per call (orion_ft_mod_modulate_device):
              ms and bytes written per second, beside the 8 TB/s HBM peak and the box's own
              streaming-read figure (orion_diag_stream_read over a 1 GiB buffer).
  synth       ft8_synth into 256 channels x 180,000 samples with 1, 8 and 32 signals per
              channel (random start symbols in [-2, 12], random base frequencies).
  demodulate  Ft8Demod over 1, 16 and 256 frames (orion_ft_demod_device, tones only and with
              the energies), beside compute_waterfall(mode="energy") over the same frames
              (79 x 8 cells per frame: the route the library had before k_ft_demod).
  ft8_decode  256 channels x 20 candidates on synthesised slots (8 decodable frames per
              channel plus Gaussian noise drawn on the device by torch) beside noise slots.

Per call: device events around one C-ABI call, after --warmup calls; median and min over
--reps calls. A modulate / synth call builds its per-signal tables on the host and uploads
them before it launches, so its figure is the call, not the kernel alone: the kernel-only
time is the difference to the wall-clock host part, which is reported too."""
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

FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND = 12000.0, 0.0, 3000.0, -2, 12, 20
N_SLOT = 180_000
SPS, TOTAL, TONES, DATA = 1920, 79, 8, 58
FRAME = SPS * TOTAL
HBM_PEAK = 8.0e12


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), statistics.median(wall)


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def stream_read_rate(warmup, reps):
    x = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    s = torch.cuda.current_stream().cuda_stream
    nb = orion_sdr.diag_stream_read(x, s)
    med, lo, _ = timed(lambda: orion_sdr.diag_stream_read(x, s), warmup, reps)
    return nb / (med * 1e-3)


def run_modulate(nf, read_rate, warmup, reps, out):
    rng = np.random.default_rng(3)
    tones = rng.integers(0, TONES, (nf, DATA)).astype(np.uint8)
    mod = orion_sdr.Ft8Mod(FS, 1000.0, 0.0, 1.0)
    iq = torch.empty((nf, FRAME), dtype=torch.complex64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L = orion_sdr._L

    def call():
        orion_sdr._check(L.orion_ft_mod_modulate_device(mod._h, tones.ctypes.data, nf, iq.data_ptr(), s))

    med, lo, wall = timed(call, warmup, reps)
    nbytes = nf * FRAME * 8
    rate = nbytes / (med * 1e-3)
    emit({"case": "ft8 modulate", "frames": nf, "reps": reps, "ms_median": round(med, 4), "ms_min": round(lo, 4),
          "host_call_ms_median": round(wall, 4), "bytes_written": nbytes, "bytes_per_s": float(f"{rate:.4g}"),
          "of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4), "stream_read_bytes_per_s": float(f"{read_rate:.4g}"),
          "of_stream_read": round(rate / read_rate, 4)}, out)


def slot_signals(nch, per_ch, rng):
    sig = np.zeros(nch * per_ch, orion_sdr.SIGNAL_DTYPE)
    sig["channel"] = np.repeat(np.arange(nch), per_ch)
    sig["offset"] = rng.integers(T_MIN, T_MAX + 1, nch * per_ch) * SPS
    sig["base_hz"] = 200.0 + 6.25 * rng.integers(0, 400, nch * per_ch)
    sig["gain"] = 1.0
    return sig


def run_synth(nch, per_ch, read_rate, warmup, reps, out):
    rng = np.random.default_rng(5)
    sig = slot_signals(nch, per_ch, rng)
    tones = rng.integers(0, TONES, (len(sig), DATA)).astype(np.uint8)
    iq = torch.empty((nch, N_SLOT), dtype=torch.complex64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L = orion_sdr._L

    def call():
        orion_sdr._check(L.orion_ft_synth_device(0, FS, sig.ctypes.data, tones.ctypes.data, len(sig), nch, N_SLOT, 0,
                                                 iq.data_ptr(), s))

    med, lo, wall = timed(call, warmup, reps)
    nbytes = nch * N_SLOT * 8
    rate = nbytes / (med * 1e-3)
    emit({"case": "ft8 synth", "nch": nch, "n_per_ch": N_SLOT, "signals_per_ch": per_ch, "reps": reps,
          "ms_median": round(med, 4), "ms_min": round(lo, 4), "host_call_ms_median": round(wall, 4),
          "table_bytes": int(len(sig) * 1696 + (nch + 1) * 4), "bytes_written": nbytes,
          "bytes_per_s": float(f"{rate:.4g}"), "of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4),
          "of_stream_read": round(rate / read_rate, 4),
          "signal_samples_per_s": float(f"{nch * per_ch * N_SLOT / (med * 1e-3):.4g}")}, out)


def run_demod(nf, warmup, reps, out):
    rng = np.random.default_rng(9)
    tones = rng.integers(0, TONES, (nf, DATA)).astype(np.uint8)
    iq = orion_sdr.Ft8Mod(FS, 1000.0, 0.0, 1.0).modulate(tones, device=True)
    iq = (iq + 0.5 * torch.view_as_complex(torch.randn((nf, FRAME, 2), device="cuda"))).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    L = orion_sdr._L
    td = torch.empty((nf, DATA), dtype=torch.uint8, device="cuda")
    en = torch.empty((nf, TOTAL, TONES), dtype=torch.float32, device="cuda")
    wf = torch.empty((nf, TOTAL, TONES), dtype=torch.float32, device="cuda")
    eng = orion_sdr.SyncEngine()

    def demod():
        orion_sdr._check(L.orion_ft_demod_device(0, FS, 1000.0, iq.data_ptr(), nf, FRAME, td.data_ptr(), None, s))

    def demod_e():
        orion_sdr._check(L.orion_ft_demod_device(0, FS, 1000.0, iq.data_ptr(), nf, FRAME, td.data_ptr(), en.data_ptr(), s))

    def waterfall():
        orion_sdr._check(L.orion_waterfall_compute_device(eng._h, iq.data_ptr(), FS, 1000.0, 6.25, SPS, TOTAL, TONES, 0,
                                                          nf, FRAME, 1, wf.data_ptr(), s))

    dmed, dlo, _ = timed(demod, warmup, reps)
    emed, elo, _ = timed(demod_e, warmup, reps)
    wmed, wlo, _ = timed(waterfall, warmup, reps)
    same = bool(torch.equal(en.view(torch.int32), wf.view(torch.int32)))
    ok = bool((td.cpu().numpy() == tones).all())
    emit({"case": "ft8 demodulate", "frames": nf, "reps": reps, "demod_ms_median": round(dmed, 4),
          "demod_ms_min": round(dlo, 4), "demod_with_energies_ms_median": round(emed, 4),
          "demod_with_energies_ms_min": round(elo, 4), "waterfall_energy_ms_median": round(wmed, 4),
          "waterfall_energy_ms_min": round(wlo, 4), "waterfall_over_demod": round(wmed / dmed, 2),
          "cell_samples_per_s": float(f"{nf * TOTAL * TONES * SPS / (dmed * 1e-3):.4g}"),
          "energies_equal_waterfall_bits": same, "tones_recovered": ok}, out)


def run_decode(nch, per_ch, noise_power, rule, warmup, reps, out):
    rng = np.random.default_rng(13)
    L = orion_sdr._L
    eng = orion_sdr.SyncEngine()
    g = torch.Generator(device="cuda").manual_seed(7)
    noise = torch.view_as_complex(torch.randn((nch, N_SLOT, 2), device="cuda", generator=g))
    slots = {"noise slot": noise.contiguous()}
    payloads = [rng.integers(0, 256, 10).astype(np.uint8).tobytes() for _ in range(nch * per_ch)]
    tones = np.stack([orion_sdr.Ft8Codec.encode(p) for p in payloads])
    sig = slot_signals(nch, per_ch, rng)
    sig["offset"] = rng.integers(0, T_MAX + 1, len(sig)) * SPS
    synth = orion_sdr.ft8_synth(sig, tones, N_SLOT, nch=nch, device=True)
    slots[f"synthesised slot ({per_ch} frames per channel, noise power {noise_power})"] = \
        (synth + float(np.sqrt(noise_power / 2.0)) * noise).contiguous()
    cand = torch.empty((nch, MAX_CAND, 3), dtype=torch.int32, device="cuda")
    count = torch.empty((nch,), dtype=torch.int32, device="cuda")
    llr = torch.empty((nch, MAX_CAND, 174), dtype=torch.float32, device="cuda")
    res = torch.empty((nch, MAX_CAND, 4), dtype=torch.int32, device="cuda")
    pick = torch.empty((nch, 4), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    geo = (nch, N_SLOT, FS, BASE_HZ, MAX_HZ, T_MIN, T_MAX, MAX_CAND)
    for name, x in slots.items():
        def decode():
            orion_sdr._check(L.orion_ft8_decode_device(eng._h, x.data_ptr(), *geo, orion_sdr._rule(rule), 20,
                                                       cand.data_ptr(), count.data_ptr(), llr.data_ptr(), res.data_ptr(),
                                                       pick.data_ptr(), s))

        med, lo, _ = timed(decode, warmup, reps)
        r = res.cpu().numpy().view(orion_sdr.RESULT_DTYPE)[..., 0]
        sent = {(int(c), p[:9] + bytes([p[9] & 0xF8])) for c, p in zip(sig["channel"], payloads)}
        good = sum(1 for ch in range(nch) for k in range(MAX_CAND)
                   if r[ch, k]["status"] == 2 and (ch, r[ch, k]["payload"].tobytes()) in sent)
        emit({"case": "ft8_decode", "input": name, "rule": rule, "nch": nch, "max_cand": MAX_CAND, "n_per_ch": N_SLOT,
              "reps": reps, "decode_ms_median": round(med, 4), "decode_ms_min": round(lo, 4),
              "slots_per_s": round(nch / (med * 1e-3), 1), "candidates_decoded": int((r["status"] == 2).sum()),
              "decoded_candidates_carrying_a_sent_payload": int(good),
              "mean_iterations": round(float(r["iterations"].mean()), 2)}, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftmod_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--signals", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--noise-power", type=float, default=10.0)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("ftmod_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    reps = max(20, a.reps)
    with open(a.out, "a") as out:
        read_rate = stream_read_rate(a.warmup, reps)
        for nf in a.frames:
            run_modulate(nf, read_rate, a.warmup, reps, out)
        for k in a.signals:
            run_synth(a.channels, k, read_rate, a.warmup, reps, out)
        for nf in a.frames:
            run_demod(nf, a.warmup, reps, out)
        for rule in ("reference", "sum_product"):
            run_decode(a.channels, 8, a.noise_power, rule, a.warmup, reps, out)
