"""Times the frame layer's coding chain on device-resident data: frame_encode_chain_batch,
frame_decode_chain_batch and the round trip of both, for the two concatenations the reference
benchmarks (tests/performance/throughput/cofdm.rs: a 96-byte payload under LDPC(n512r12) +
BCH(t = 8), and under convolutional K5 r1/2 + RS(60,52)), at --frames (default 1, 256, 4096)
frames per call. One JSON line per case, appended to --out (default profiles/frame_bench.jsonl).

Two records per case. "frame_chain" times the chain between payload bytes and coded bits / LLRs
alone: CRC, whitener, both codes, their interleavers and the glue kernels of csrc/k_frame.hip,
in frames/s and payload bit/s. "frame" times the whole frame as the reference's benchmark does
(n_fft 64, cp 8, 62 data carriers, QPSK, frames of 2584 and 1936 samples):
OfdmFrameMod.modulate_frames, the known-start OfdmFrameDemod.decode_frames and the round trip, in
Msps as the reference counts them, frame samples over time. The reference's published figures
(docs/performance.md:253-269, an M2 Pro: ~83 / ~54 Msps modulate / decode for LDPC + BCH, ~90 /
~31 Msps for convolutional + RS) are quoted in each record for context only.

Per case: device events around --iters back-to-back calls, after a warm-up of the same shape;
median and min of the per-call time over --reps such windows. The decode input is BPSK plus
Gaussian noise at --sigma (llr = 2 y / sigma^2), where the inner decoders have work to do. Beside
each figure: every launch of the call timed alone the same way (the share of the glue kernels
against the codes), one host thread of the library's own encode_chain / decode_chain (wall
clock, through ctypes, at most --host-frames frames), and whether its output is the device's.
Nothing is asserted about speed."""
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

PAYLOAD = 96
WORKLOADS = {
    # name: (scheme arguments, frame samples and the reference's Msps, for context)
    "ldpc_n512r12_bch_t8": (dict(outer=("bch", 8), inner=("ldpc", "n512r12")), 2584, (83, 54)),
    "conv_k5_r12_rs_60_52": (dict(outer=("rs", 60, 8), inner=("conv", "1/2", "k5")), 1936, (90, 31)),
}


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


def stages(sch, kw, plan, d_pay, d_llr, a):
    """Every launch of the two calls alone, on the tensors the launch before it made."""
    out, keep = {}, {}

    def t(name, fn):
        keep[name] = fn()
        out[name + "_us"] = us(timed(fn, a.warmup, a.reps, a.iters)[0])
        return keep[name]

    outer, inner = kw["outer"], kw["inner"]
    ns = int(d_pay.shape[0])

    def inner_encode(bits):
        if inner[0] == "ldpc":
            return O.ldpc_family_encode_batch(bits, inner[1])
        return O.conv_encode_batch(bits, inner[1], inner[2])

    if outer[0] == "bch":
        x = t("pack", lambda: O.frame_pack_batch(d_pay, sch))
        x = t("outer_encode", lambda: O.bch_encode_batch(x, outer[1]))
    else:
        n, k = outer[1], outer[1] - outer[2]
        ncw = -(-plan.framed_bytes // k)
        x = t("pack", lambda: O.frame_pack_batch(d_pay, sch, out_bytes=True))
        padded = torch.nn.functional.pad(x, (0, ncw * k - int(x.shape[1]))).reshape(ns, ncw, k).contiguous()
        y = t("outer_encode", lambda: O.rs_encode_batch(padded, n, outer[2]))
        x = t("bytes_to_bits", lambda: O.frame_bytes_to_bits_batch(y.reshape(ns, ncw * n)))
    x = t("inner_encode", lambda: inner_encode(x))
    t("coded_bits", lambda: O.frame_coded_bits_batch(x, sch))
    unsat = None
    if inner[0] == "ldpc":
        r = t("inner_decode", lambda: O.ldpc_family_decode_batch(d_llr, inner[1]))
        bits, unsat = r[0], r[1]
    else:
        bits = t("inner_decode", lambda: O.conv_viterbi_batch(d_llr, plan.outer_il_bits, inner[1], inner[2]))
    trimmed = bits[:, :plan.outer_coded_bits].contiguous()
    if outer[0] == "bch":
        m = t("outer_decode", lambda: O.bch_decode_batch(trimmed, outer[1]))
        t("unpack", lambda: O.frame_unpack_batch(m[0], PAYLOAD, sch, unsat=unsat, status=m[1]))
    else:
        m = t("outer_decode", lambda: O.rs_decode_batch(trimmed, outer[1], outer[2], bits=True))
        flat = m[0].reshape(ns, -1)
        t("unpack", lambda: O.frame_unpack_batch(flat, PAYLOAD, sch, in_bytes=True, unsat=unsat, status=m[1]))
    return out


def run(name, frames, a, out):
    kw, samples, ref = WORKLOADS[name]
    sch = O.FrameScheme(**kw)
    plan = O.block_plan(PAYLOAD, sch)
    rng = np.random.default_rng([0xF4A, frames])
    pay = rng.integers(0, 256, (frames, PAYLOAD), dtype=np.uint8)
    nh = min(frames, a.host_frames)
    t0 = time.perf_counter()
    h_coded = np.stack([O.encode_chain(p, sch) for p in pay[:nh]])
    h_enc = (time.perf_counter() - t0) / nh
    d_pay = torch.from_numpy(pay).cuda()
    res = {}

    def enc():
        res["c"] = O.frame_encode_chain_batch(d_pay, sch)

    e_med, e_min = timed(enc, a.warmup, a.reps, a.iters)
    coded = res["c"].cpu().numpy()
    y = (1.0 - 2.0 * coded) + a.sigma * rng.standard_normal(coded.shape)
    llr = (2.0 * y / a.sigma ** 2).astype(np.float32)
    t0 = time.perf_counter()
    h_out = [O.decode_chain(row, PAYLOAD, sch) for row in llr[:nh]]
    h_dec = (time.perf_counter() - t0) / nh
    d_llr = torch.from_numpy(llr).cuda()

    def dec():
        res["d"] = O.frame_decode_chain_batch(d_llr, PAYLOAD, sch)

    d_med, d_min = timed(dec, a.warmup, a.reps, a.iters)

    def trip():  # payload -> coded bits -> clean LLRs made on the device -> payload, nothing leaves it
        c = O.frame_encode_chain_batch(d_pay, sch)
        res["t"] = O.frame_decode_chain_batch(4.0 - 8.0 * c.to(torch.float32), PAYLOAD, sch)

    t_med, t_min = timed(trip, a.warmup, a.reps, a.iters)
    g = {k: v.cpu().numpy() for k, v in res["d"].items()}
    same = np.array_equal(coded[:nh], h_coded) and all(
        np.array_equal(g["payload"][k], o.bytes) and bool(g["crc_ok"][k]) == o.crc_ok and
        bool(g["inner_ok"][k]) == o.inner_ok and bool(g["outer_ok"][k]) == o.outer_ok for k, o in enumerate(h_out))
    rec = {"case": "frame_chain", "workload": name, "payload_bytes": PAYLOAD, "frames": frames,
           "coded_bits": plan.coded_bits, "sigma": a.sigma, "reps": a.reps, "iters": a.iters,
           "encode_us_median": us(e_med), "encode_us_min": us(e_min), "encode_frames_per_s": float(f"{frames / (e_med * 1e-3):.4g}"),
           "decode_us_median": us(d_med), "decode_us_min": us(d_min), "decode_frames_per_s": float(f"{frames / (d_med * 1e-3):.4g}"),
           "round_trip_us_median": us(t_med), "round_trip_us_min": us(t_min),
           "round_trip_frames_per_s": float(f"{frames / (t_med * 1e-3):.4g}"),
           "decode_payload_mbit_per_s": float(f"{frames * PAYLOAD * 8 / (d_med * 1e-3) / 1e6:.4g}"),
           "crc_failures": int((~g["crc_ok"]).sum()), "inner_not_converged": int((~g["inner_ok"]).sum()),
           "round_trip_all_valid": bool(res["t"]["valid"].all().item()),
           "host_frames": nh, "host_encode_us_per_frame": round(h_enc * 1e6, 3),
           "host_decode_us_per_frame": round(h_dec * 1e6, 3), "host_equals_device": bool(same),
           "launches_us": stages(sch, kw, plan, d_pay, d_llr, a),
           "context_only": {"whole_frame_samples": samples, "reference_m2_pro_msps_modulate_decode": list(ref),
                            "note": "the OFDM symbol layer and the preamble are not in this record's times"}}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


DATA62 = np.array([i for i in range(-31, 32) if i != 0], np.int32)  # n_fft 64, cp 8, 62 data carriers


def run_frames(name, frames, a, out):
    """The whole frame: OfdmFrameMod.modulate_frames, OfdmFrameDemod.decode_frames (known start)
    and the round trip, in Msps as the reference counts them: frame samples over time."""
    kw, samples, ref = WORKLOADS[name]
    cfg = O.OfdmConfig(64, 8, DATA62, np.zeros(0, np.int32), np.zeros(0, np.complex64), 1e6, 0.0, 1.0, "qpsk")
    table = O.McsTable([O.Mcs("qpsk", kw["inner"], kw["outer"])])
    pre = O.OfdmPreamble(2, 32).with_training_symbol(64, 8)
    mod, dem = O.OfdmFrameMod(cfg, table, pre), O.OfdmFrameDemod(cfg, table)
    assert mod.frame_len(0, PAYLOAD) == samples
    rng = np.random.default_rng([0xF4B, frames])
    pay = rng.integers(0, 256, (frames, PAYLOAD), dtype=np.uint8)
    seq = np.arange(frames, dtype=np.int64)
    nh = min(frames, a.host_frames)
    t0 = time.perf_counter()
    h_iq = [mod.modulate_frame(O.FramePacket(O.FrameMetadata(int(seq[k]), 0), pay[k])) for k in range(nh)]
    h_mod = (time.perf_counter() - t0) / nh
    d_pay, d_seq = torch.from_numpy(pay).cuda(), torch.from_numpy(seq).cuda()
    res = {}

    def tx():
        res["iq"] = mod.modulate_frames(d_pay, 0, sequence_nums=d_seq)

    m_med, m_min = timed(tx, a.warmup, a.reps, a.iters)
    iq = res["iq"].cpu().numpy()
    same_tx = all(np.array_equal(iq[k].view(np.uint32), h_iq[k].view(np.uint32)) for k in range(nh))
    body = iq[:, pre.total_len:]
    noise = (rng.standard_normal(body.shape) + 1j * rng.standard_normal(body.shape)) * a.body_sigma
    rx = (body + noise.astype(np.complex64)).astype(np.complex64)
    t0 = time.perf_counter()
    h_ok = []
    for k in range(nh):
        try:
            h_ok.append(np.array_equal(dem.decode(rx[k]).payload, pay[k]))
        except O.RxError:
            h_ok.append(False)
    h_dec = (time.perf_counter() - t0) / nh
    d_rx = torch.from_numpy(rx).cuda()

    def rxf():
        res["out"] = dem.decode_frames(d_rx)

    d_med, d_min = timed(rxf, a.warmup, a.reps, a.iters)

    def trip():
        x = mod.modulate_frames(d_pay, 0, sequence_nums=d_seq)
        res["t"] = dem.decode_frames(x[:, pre.total_len:].contiguous())

    t_med, t_min = timed(trip, a.warmup, a.reps, a.iters)
    g = res["out"]
    same_rx = all((g["error"][k] == 0) == h_ok[k] for k in range(nh))
    msps = lambda ms: float(f"{frames * samples / (ms * 1e-3) / 1e6:.4g}")  # noqa: E731
    rec = {"case": "frame", "workload": name, "payload_bytes": PAYLOAD, "frames": frames, "frame_samples": samples,
           "body_sigma": a.body_sigma, "reps": a.reps, "iters": a.iters,
           "modulate_us_median": us(m_med), "modulate_us_min": us(m_min), "modulate_msps": msps(m_med),
           "modulate_frames_per_s": float(f"{frames / (m_med * 1e-3):.4g}"),
           "decode_us_median": us(d_med), "decode_us_min": us(d_min), "decode_msps": msps(d_med),
           "decode_frames_per_s": float(f"{frames / (d_med * 1e-3):.4g}"),
           "round_trip_us_median": us(t_med), "round_trip_us_min": us(t_min), "round_trip_msps": msps(t_med),
           "decode_errors": int((g["error"] != 0).sum()), "round_trip_errors": int((res["t"]["error"] != 0).sum()),
           "host_frames": nh, "host_modulate_us_per_frame": round(h_mod * 1e6, 3),
           "host_modulate_msps": float(f"{samples / h_mod / 1e6:.4g}"),
           "host_decode_us_per_frame": round(h_dec * 1e6, 3), "host_decode_msps": float(f"{samples / h_dec / 1e6:.4g}"),
           "host_equals_device": bool(same_tx and same_rx),
           "note": "decode_frames includes its one device-to-host copy of the header fields and the host-side grouping; "
                   "the host figures are the library's Python-composed host path on one thread",
           "context_only": {"reference_m2_pro_msps_modulate_decode": list(ref)}}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 256, 4096])
    ap.add_argument("--sigma", type=float, default=0.7)
    ap.add_argument("--body-sigma", type=float, default=0.06)
    ap.add_argument("--host-frames", type=int, default=256)
    a = ap.parse_args()
    if O.device_count() < 1:
        raise SystemExit("frame_bench: no HIP device visible (timings are taken on the GPU only)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for name in WORKLOADS:
            for frames in a.frames:
                run(name, frames, a, out)
                run_frames(name, frames, a, out)
