"""Times the OFDM symbol layer's kernels (csrc/k_ofdm.hip) on device-resident data. One JSON
line per case, appended to --out (default profiles/ofdm_bench.jsonl).

The workload is the reference's throughput harness configuration
(tests/performance/throughput/ofdm.rs): n_fft 1024, cp 128, 1022 data carriers, QPSK and
QAM-64, here 256 symbols x 64 channels, resident. Per constellation: the modulator
(ofdm_modulate_batch), the demodulator with the hard bits from the same launch
(ofdm_demodulate_batch), and the round trip (both, back to back), in Msps of IQ and as
achieved bytes per second against the algorithmic bytes (modulator: the bits in plus 9216 B of
IQ out per symbol; demodulator: 9216 B in plus the soft symbols and the bits out). Then the
stand-alone transform at 64 / 1024 / 2048 / 4096 points over 16384 symbols (8 B in and 8 B out
per point).

Per case: device events around one call on resident torch tensors, after --warmup calls;
median and min over --reps calls. Beside each, the library's host scalar path (one thread of
the same machine, wall clock, through ctypes) on --host-symbols of the symbols."""
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


def host_timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def emit(out, rec):
    print(json.dumps(rec))
    out.write(json.dumps(rec) + "\n")


def run_link(order, nch, nsym, warmup, reps, host_symbols, out):
    z32, zc = np.zeros(0, np.int32), np.zeros(0, np.complex64)
    cfg = orion_sdr.OfdmConfig(1024, 128, z32, z32, zc, 1e6, 0.0, 1.0, order, edge_guard=0)
    assert cfg.num_data_carriers == 1022
    mod, dem = orion_sdr.OfdmMod(cfg), orion_sdr.OfdmDemod(cfg, None)
    bps, slen, nd = cfg.bits_per_ofdm_symbol, cfg.samples_per_ofdm_symbol, cfg.num_data_carriers
    bits = np.random.default_rng(1).integers(0, 2, (nch, nsym * bps)).astype(np.uint8)
    dbits = torch.from_numpy(bits).cuda()
    iq = orion_sdr.ofdm_modulate_batch(mod, dbits)
    soft, back, _ = orion_sdr.ofdm_demodulate_batch(dem, iq)
    ok = bool(torch.equal(back, dbits))
    nsamp = nch * nsym * slen
    cases = {
        "mod": (lambda: orion_sdr.ofdm_modulate_batch(mod, dbits), nch * nsym * (bps + slen * 8)),
        "demod_decide": (lambda: orion_sdr.ofdm_demodulate_batch(dem, iq), nch * nsym * (slen * 8 + nd * 8 + bps)),
        "round_trip": (lambda: orion_sdr.ofdm_demodulate_batch(dem, orion_sdr.ofdm_modulate_batch(mod, dbits)),
                       nch * nsym * (2 * bps + 2 * slen * 8 + nd * 8)),
    }
    hs = min(host_symbols, nsym)
    hb = np.ascontiguousarray(bits[0, : hs * bps])
    hiq = mod.modulate_host(hb)
    host = {
        "mod": host_timed(lambda: mod.modulate_host(hb)),
        "demod_decide": host_timed(lambda: orion_sdr.ofdm_decide(order, dem.process_host(hiq))),
    }
    host["round_trip"] = host["mod"] + host["demod_decide"]
    for name, (fn, nbytes) in cases.items():
        med, mn = timed(fn, warmup, reps)
        emit(out, {"case": f"ofdm_{name}", "constellation": order, "n_fft": 1024, "cp_len": 128, "channels": nch,
                   "symbols": nsym, "median_ms": med, "min_ms": mn, "msps_iq": nsamp / med / 1e3,
                   "algorithmic_bytes": nbytes, "gb_per_s": nbytes / med / 1e6, "round_trip_bits_ok": ok,
                   "host_scalar_ms": host[name], "host_symbols": hs, "host_msps_iq": hs * slen / host[name] / 1e3})


def run_fft(n, batch, warmup, reps, host_symbols, out):
    x = (np.random.default_rng(2).standard_normal((batch, 2 * n)).astype(np.float32)).view(np.complex64)
    d = torch.from_numpy(x).cuda()
    f = orion_sdr.FftBlock(n)
    med, mn = timed(lambda: f.process_batch(d), warmup, reps)
    hs = min(host_symbols, batch)
    hx = np.ascontiguousarray(x[:hs]).reshape(-1)
    hms = host_timed(lambda: orion_sdr.fft_host(hx, n))
    same = bool(np.array_equal(f.process_batch(d)[:hs].cpu().numpy().reshape(-1).view(np.uint64),
                               orion_sdr.fft_host(hx, n).view(np.uint64)))
    emit(out, {"case": "fft", "n_fft": n, "batch": batch, "median_ms": med, "min_ms": mn,
               "msps": batch * n / med / 1e3, "algorithmic_bytes": batch * n * 16, "gb_per_s": batch * n * 16 / med / 1e6,
               "host_scalar_ms": hms, "host_symbols": hs, "host_msps": hs * n / hms / 1e3, "bits_equal_host": same})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ofdm_bench.jsonl"))
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--symbols", type=int, default=256)
    ap.add_argument("--fft-batch", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-symbols", type=int, default=256)
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("ofdm_bench: no HIP device visible")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as out:
        for order in ("qpsk", "qam64"):
            run_link(order, a.channels, a.symbols, a.warmup, a.reps, a.host_symbols, out)
        for n in (64, 1024, 2048, 4096):
            run_fft(n, a.fft_batch, a.warmup, a.reps, a.host_symbols, out)


if __name__ == "__main__":
    main()
