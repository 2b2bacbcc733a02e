"""Times the PSK31 kernels of csrc/k_psk31.hip on device-resident data. One JSON line per
case, appended to --out (default profiles/psk31_bench.jsonl).

The demodulator bank (k_psk31_demod): a 30 s buffer at 8 kHz (240000 samples per channel,
Gaussian noise: the loop's work does not depend on the data) for 1, 16 and 256 channels, 97
BPSK31 streams per channel at 31.25 Hz spacing from 31.25 Hz up (all with a rotator), each
with room for every symbol; reported as time per call and as symbols per second. --single
adds a bank of one stream (what Bpsk31Demod.process costs). Beside each, the library's host
scalar demodulator (orion_psk31_demod_process, one thread, wall clock) timed on a sample of at
most --bank-host-streams of the streams, spread over the list; the figure for all streams is
that time scaled to the stream count, and is named as extrapolated.

psk31_sync (orion_psk31_sync_device) on the same buffer length with five carriers and noise
per channel, 0-3000 Hz, 10 candidates of 1024 bits, for the same channel counts: the whole
call, and the waterfall, the search and the candidates' demodulation each timed alone; beside
the search, the library's host search on the downloaded waterfall, one thread.

The synthesiser and modulator entries (orion_psk31_synth_device, modulate_batch on a device
tensor): wall clock around one call and a synchronise, since their cost is the host's plan
build, upload and launch; a small and a larger call of each.

The batched QPSK31 Viterbi decode (k_psk31_viterbi) on
device-resident soft symbols: 1, 64 and 4096 streams of 1024 symbols (coded random bits
as DQPSK phasors plus Gaussian noise of deviation 0.5).

Per launch: device events around one orion_psk31_viterbi_device call (its scratch is
allocated once, outside the timed region), after --warmup calls; median and min over --reps
launches. Beside each, the library's own host scalar decoder (orion_psk31_viterbi_host, one
thread of the GPU box's host, wall clock, through ctypes) on the same streams (at most
--host-streams of them), and whether its bits equal the device's."""
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


def streams(n, n_syms, sigma):
    rng = np.random.default_rng(31)
    exp = orion_sdr.psk31_tables()[2]
    base = []
    for _ in range(min(n, 64)):  # 64 distinct bit streams, repeated with fresh noise
        coded = orion_sdr.conv_encode(rng.integers(0, 2, n_syms).astype(np.uint8)).reshape(n_syms, 2)
        base.append(exp[coded[:, 0] * 2 + coded[:, 1]].reshape(-1))
    out = np.stack([base[k % len(base)] for k in range(n)])
    return (out + rng.normal(0.0, sigma, out.shape)).astype(np.float32)


def run_viterbi(n, n_syms, sigma, warmup, reps, host_streams, out):
    x = streams(n, n_syms, sigma)
    d = torch.from_numpy(x).cuda()
    bits = torch.empty((n, n_syms), dtype=torch.uint8, device="cuda")
    L = orion_sdr._L
    wb = int(L.orion_psk31_viterbi_work_bytes(n, n_syms))
    work = torch.empty(wb // 4, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def dev():
        orion_sdr._check(L.orion_psk31_viterbi_device(d.data_ptr(), n, n_syms, bits.data_ptr(), work.data_ptr(), wb, s))

    med, lo = timed(dev, warmup, reps)
    got = bits.cpu().numpy()
    nh = min(n, host_streams)
    hb = np.zeros(n_syms, np.uint8)
    same = True
    t0 = time.perf_counter()
    for k in range(nh):
        orion_sdr._check(L.orion_psk31_viterbi_host(x[k].ctypes.data, n_syms, hb.ctypes.data))
        same = same and hb.tobytes() == got[k].tobytes()
    dt = time.perf_counter() - t0
    rec = {"case": "psk31_viterbi", "sigma": sigma, "nstreams": n, "n_syms": n_syms, "reps": reps,
           "ms_median": round(med, 4), "ms_min": round(lo, 4), "symbols_per_s": float(f"{n * n_syms / (med * 1e-3):.4g}"),
           "work_bytes": wb, "host_streams": nh, "host_ms": round(dt * 1e3, 3),
           "host_ms_per_stream": round(dt * 1e3 / nh, 4), "host_symbols_per_s": float(f"{nh * n_syms / dt:.4g}"),
           "host_equals_device": bool(same)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def run_bank(nch, per_ch, n, warmup, reps, host_streams, out):
    fs = 8000.0
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.view_as_complex(torch.randn((nch, n, 2), device="cuda", generator=g))
    ns = nch * per_ch
    cap = n // 256 + 2
    rec = np.zeros(ns, orion_sdr.PSK31_STREAM_DTYPE)
    rec["mode"] = 0
    rec["channel"] = np.repeat(np.arange(nch), per_ch)
    rec["rf_hz"] = np.tile(31.25 * (1 + np.arange(per_ch)), nch)
    rec["gain"] = 1.0
    rec["out_cap"] = cap
    bank = orion_sdr.Psk31DemodBank(fs, rec, nch)
    soft = torch.zeros((ns, cap), dtype=torch.float32, device="cuda")
    bits = torch.zeros((ns, cap), dtype=torch.uint8, device="cuda")
    rep = torch.zeros((ns, 2), dtype=torch.int64, device="cuda")
    L = orion_sdr._L
    s = torch.cuda.current_stream().cuda_stream

    def dev():
        orion_sdr._check(L.orion_psk31_demod_bank_process_device(bank._h, x.data_ptr(), nch, n, soft.data_ptr(), cap,
                                                                 bits.data_ptr(), rep.data_ptr(), s))

    med, lo = timed(dev, warmup, reps)
    syms = int(rep[:, 1].sum().item())
    # the host scalar demodulator, timed on a sample of the streams (at most host_streams of
    # them, spread over the list: low and high carriers, first and last channels)
    pick = np.unique(np.linspace(0, ns - 1, min(ns, host_streams)).astype(int))
    rows = {int(ch): np.ascontiguousarray(x[int(ch)].cpu().numpy()) for ch in np.unique(rec["channel"][pick])}
    demods = [orion_sdr.Bpsk31Demod(fs, float(rec["rf_hz"][k]), 1.0) for k in pick]
    t0 = time.perf_counter()
    hsyms = 0
    for k, d in zip(pick, demods):
        hsoft, nread = d.process_host(rows[int(rec["channel"][k])], cap)
        hsyms += hsoft.size
    dt = time.perf_counter() - t0
    rec_out = {"case": "psk31_demod_bank", "nch": nch, "streams_per_ch": per_ch, "nstreams": ns, "n_per_ch": n,
               "reps": reps, "ms_median": round(med, 4), "ms_min": round(lo, 4), "symbols_per_call": syms,
               "symbols_per_s": float(f"{syms / (med * 1e-3):.4g}"),
               "stream_samples_per_s": float(f"{ns * n / (med * 1e-3):.4g}"), "host_streams_timed": int(pick.size),
               "host_ms_timed": round(dt * 1e3, 3), "host_ms_per_stream": round(dt * 1e3 / pick.size, 4),
               "host_symbols_per_s": float(f"{hsyms / dt:.4g}"), "host_in_read": nread,
               "host_ms_all_streams_extrapolated": round(dt * 1e3 / pick.size * ns, 1)}
    print(json.dumps(rec_out), flush=True)
    out.write(json.dumps(rec_out) + "\n")


def run_sync(nch, n, warmup, reps, out):
    """psk31_sync on a 30 s buffer at 8 kHz, 0-3000 Hz (97 bins), 10 candidates of 1024 bits:
    the whole call, and the waterfall, the search and the candidates' demodulation each alone
    (the demodulation as a bank of the streams the sync call found)."""
    fs, base_hz, max_hz, max_cand, n_bits, sps = 8000.0, 0.0, 3000.0, 10, 1024, 256
    g = torch.Generator(device="cuda").manual_seed(32)
    x = torch.view_as_complex(0.05 * torch.randn((nch, n, 2), device="cuda", generator=g))
    # five carriers per channel so that the search has runs to find and the bank work to do
    t = torch.arange(n, device="cuda", dtype=torch.float64)
    for f in (500.0, 1000.0, 1500.0, 2000.0, 2500.0):
        x += torch.exp(2j * np.pi * f / fs * t).to(torch.complex64)[None, :]
    num_syms, num_bins = n // sps, 97
    L, eng = orion_sdr._L, orion_sdr._sync_engine()
    s = torch.cuda.current_stream().cuda_stream
    wf = torch.empty((nch, num_syms, num_bins), dtype=torch.float32, device="cuda")
    cand = torch.zeros((nch, max_cand, 3), dtype=torch.int32, device="cuda")
    count = torch.zeros(nch, dtype=torch.int32, device="cuda")
    soft = torch.zeros((nch, max_cand, n_bits + 2), dtype=torch.float32, device="cuda")
    rep = torch.zeros((nch, max_cand, 2), dtype=torch.int64, device="cuda")

    def whole():
        orion_sdr._check(L.orion_psk31_sync_device(eng._h, x.data_ptr(), nch, n, fs, base_hz, max_hz, 8, 6.0, n_bits,
                                                   max_cand, cand.data_ptr(), count.data_ptr(), soft.data_ptr(),
                                                   rep.data_ptr(), s))

    def waterfall():
        orion_sdr._check(L.orion_waterfall_compute_device(eng._h, x.data_ptr(), fs, base_hz, 31.25, sps, num_syms, num_bins,
                                                          0, nch, n, 0, wf.data_ptr(), s))

    def search():
        orion_sdr._check(L.orion_psk31_find_carriers_device(eng._h, wf.data_ptr(), nch, num_syms, num_bins, 8, 6.0,
                                                            max_cand, cand.data_ptr(), count.data_ptr(), s))

    wmed, wlo = timed(whole, warmup, reps)
    fmed, flo = timed(waterfall, warmup, reps)
    smed, slo = timed(search, warmup, reps)
    hc = cand.cpu().numpy().view(orion_sdr.CANDIDATE_DTYPE)[..., 0]
    hn = count.cpu().numpy().view(np.uint32)
    recs = [(0, ch, float(np.float32(base_hz) + np.float32(hc[ch, k]["freq_bin"]) * np.float32(31.25)), 1.0,
             int(hc[ch, k]["time_sym"]) * sps, 0, n_bits + 2) for ch in range(nch) for k in range(int(hn[ch]))]
    dmed = dlo = 0.0
    if recs:
        bank = orion_sdr.Psk31DemodBank(fs, np.array(recs, orion_sdr.PSK31_STREAM_DTYPE), nch)
        bsoft = torch.zeros((len(recs), n_bits + 2), dtype=torch.float32, device="cuda")
        brep = torch.zeros((len(recs), 2), dtype=torch.int64, device="cuda")

        def demod():
            orion_sdr._check(L.orion_psk31_demod_bank_reset(bank._h))
            orion_sdr._check(L.orion_psk31_demod_bank_process_device(bank._h, x.data_ptr(), nch, n, bsoft.data_ptr(),
                                                                     n_bits + 2, None, brep.data_ptr(), s))

        dmed, dlo = timed(demod, warmup, reps)
    # the host search on the downloaded waterfall, one thread
    hwf = wf.cpu().numpy()
    t0 = time.perf_counter()
    orion_sdr.psk31_find_carriers(hwf, 8, 6.0, max_cand)
    ht = time.perf_counter() - t0
    rec = {"case": "psk31_sync", "nch": nch, "n_per_ch": n, "num_bins": num_bins, "max_cand": max_cand, "n_bits": n_bits,
           "reps": reps, "candidates": int(hn.sum()), "sync_ms_median": round(wmed, 4), "sync_ms_min": round(wlo, 4),
           "waterfall_ms_median": round(fmed, 4), "waterfall_ms_min": round(flo, 4), "search_ms_median": round(smed, 4),
           "search_ms_min": round(slo, 4), "candidate_demod_ms_median": round(dmed, 4),
           "candidate_demod_ms_min": round(dlo, 4), "host_search_ms_one_thread": round(ht * 1e3, 3)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


def wall_timed(fn, warmup, reps):
    """Wall clock around one call and a synchronise, in microseconds: the host's part of an entry
    (plan build, upload, launch) is what these entries cost, and device events do not see it."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.median(us), 1), round(min(us), 1)


def run_entries(warmup, reps, out):
    """psk31_synth and modulate_batch on device tensors: a small and a larger call of each."""
    rng = np.random.default_rng(3)
    fs, sps = 8000.0, 256
    for nch, per_ch, nbits in ((1, 1, 64), (16, 8, 256)):
        sig = np.zeros(nch * per_ch, orion_sdr.PSK31_SIGNAL_DTYPE)
        for k in range(sig.size):
            sig[k] = (k % nch, k % 2, 100 * k, 500.0 + 31.25 * k, 0.5, 0)
        bits = [rng.integers(0, 2, nbits).astype(np.uint8) for _ in range(sig.size)]
        n = (nbits + 8) * sps
        buf = torch.zeros((nch, n), dtype=torch.complex64, device="cuda")
        med, lo = wall_timed(lambda: orion_sdr.psk31_synth(sig, bits, n, nch=nch, fs=fs, out=buf), warmup, reps)
        rec = {"case": "psk31_synth call", "nch": nch, "signals": int(sig.size), "n_bits": nbits, "reps": reps,
               "wall_us_median": med, "wall_us_min": lo}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")
    for ns, n in ((1, 64), (64, 256)):
        b = rng.integers(0, 2, (ns, n)).astype(np.uint8)
        m = orion_sdr.Qpsk31Mod(fs, 1000.0, 0.7)
        med, lo = wall_timed(lambda: m.modulate_batch(b, device=True), warmup, reps)
        rec = {"case": "psk31 modulate_batch call", "nstreams": ns, "n_bits": n, "reps": reps, "wall_us_median": med,
               "wall_us_min": lo}
        print(json.dumps(rec), flush=True)
        out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psk31_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--n-syms", type=int, default=1024)
    ap.add_argument("--host-streams", type=int, default=256)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--streams-per-ch", type=int, default=97)
    ap.add_argument("--samples", type=int, default=240000)
    ap.add_argument("--bank-host-streams", type=int, default=97, help="streams the host demodulator is timed on")
    ap.add_argument("--single", action="store_true", help="also time a bank of one stream")
    a = ap.parse_args()
    if orion_sdr.device_count() < 1:
        raise SystemExit("psk31_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.single:
            run_bank(1, 1, a.samples, a.warmup, max(20, a.reps), a.bank_host_streams, out)
        for nch in a.channels:
            run_bank(nch, a.streams_per_ch, a.samples, a.warmup, max(20, a.reps), a.bank_host_streams, out)
        for nch in a.channels:
            run_sync(nch, a.samples, a.warmup, max(20, a.reps), out)
        for n in a.sizes:
            run_viterbi(n, a.n_syms, 0.5, a.warmup, max(20, a.reps), a.host_streams, out)
        run_entries(a.warmup, max(50, a.reps), out)
