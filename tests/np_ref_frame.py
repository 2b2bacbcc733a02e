"""Independent numpy restatement of the reference's frame coding chain (test infrastructure):
the frame CRCs (src/codec/crc.rs:89-130), the bit/byte and header helpers, build_scrambler /
scramble_bytes / scramble_bits, block_plan and encode_chain (src/modulate/ofdm_frame.rs:204-682),
apply_pn_to_llrs and decode_chain with its ChainOutcome (src/demodulate/ofdm_frame.rs:351-779).
Written from those files over the other restatements (np_ref_bch, np_ref_ldpc_family,
np_ref_fec, np_ref_rs), not from csrc/frame.cpp.

A scheme is a dict with the keys of orion_sdr.FrameScheme's arguments: crc "none" / "crc16" /
"crc32"; outer None, ("bch", t), ("rs", n, n_parity); inner None, ("ldpc", name), ("conv", rate,
code); outer_interleaver / inner_interleaver None, ("block", rows, cols), ("forney", branches,
depth); scrambler None, "dvbt", ("additive", poly, width, seed | "per_frame"); scrambler_pos
"before_outer" / "after_inner"."""
import functools

import numpy as np

import np_ref_bch as RB
import np_ref_fec as RF
import np_ref_ldpc_family as RL
import np_ref_rs as RR

BCH_INFO_BITS = 120
HEADER_FIELD_BYTES = 14
MALFORMED_HEADER = 2
CRC_LEN = {"none": 0, "crc16": 2, "crc32": 4}


def scheme(crc="crc32", outer=None, inner=None, outer_interleaver=None, inner_interleaver=None, scrambler=None,
           scrambler_pos="before_outer"):
    return dict(crc=crc, outer=outer, inner=inner, outer_interleaver=outer_interleaver,
                inner_interleaver=inner_interleaver, scrambler=scrambler, scrambler_pos=scrambler_pos)


# ---- crc.rs:89-130 --------------------------------------------------------------------------
def crc16(data):
    crc = 0xFFFF
    for byte in bytes(data):
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def crc32(data):
    crc = 0xFFFFFFFF
    for byte in bytes(data):
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ 0xEDB88320 if crc & 1 else crc >> 1
    return crc ^ 0xFFFFFFFF


def append_crc(crc, data):
    data = bytes(np.asarray(data, np.uint8))
    if crc == "crc16":
        data += crc16(data).to_bytes(2, "big")
    elif crc == "crc32":
        data += crc32(data).to_bytes(4, "big")
    return np.frombuffer(data, np.uint8).copy()


def check_and_strip_crc(crc, data):
    data = bytes(np.asarray(data, np.uint8))
    clen = CRC_LEN[crc]
    if len(data) < clen:
        return None
    payload, tail = data[:len(data) - clen], data[len(data) - clen:]
    ok = True if crc == "none" else (crc16(payload) if crc == "crc16" else crc32(payload)).to_bytes(clen, "big") == tail
    return np.frombuffer(payload, np.uint8).copy(), ok


def pack_header_fields(mcs_index, payload_len, sequence_num, flags, scrambler_seed):
    return np.frombuffer(bytes([mcs_index]) + payload_len.to_bytes(4, "big") + sequence_num.to_bytes(4, "big") +
                         bytes([flags]) + scrambler_seed.to_bytes(4, "big"), np.uint8).copy()


# ---- scramblers, ofdm_frame.rs:266-312, 650-665 ---------------------------------------------
def build_scrambler(sch, per_frame_seed):
    """(taps, width, seed) of the PnScrambler, or None."""
    sc = sch["scrambler"]
    if sc is None or sc == "dvbt":
        return None
    _, poly, width, seed = sc
    raw = per_frame_seed if seed == "per_frame" else seed
    mask = 0xFFFFFFFF if width >= 32 else (1 << width) - 1
    m = raw & mask
    return poly, width, 1 if m == 0 else m


def scramble_bytes(sch, per_frame_seed, data):
    if sch["scrambler"] == "dvbt":
        return RR.Dispersal().feed(data)
    s = build_scrambler(sch, per_frame_seed)
    return RR.pn_scramble(*s, data) if s else np.asarray(data, np.uint8).copy()


def pack_bits_padded(bits):
    bits = np.asarray(bits, np.uint8)
    return RR.bits_to_bytes(np.concatenate([bits, np.zeros(-len(bits) % 8, np.uint8)]))


def scramble_bits(s, bits):
    """s = build_scrambler's triple: pack (zero-padded), XOR the PN, unpack, trim."""
    return RR.bytes_to_bits(RR.pn_scramble(*s, pack_bits_padded(bits)))[:len(bits)]


def apply_pn_to_llrs(s, llr):
    llr = np.asarray(llr, np.float32).copy()
    pn = RR.bytes_to_bits(RR.pn_scramble(*s, np.zeros(-(-len(llr) // 8), np.uint8)))[:len(llr)]
    u = llr.view(np.uint32)
    u[pn != 0] ^= np.uint32(0x80000000)  # -x
    return llr


# ---- block_plan, ofdm_frame.rs:320-438 ------------------------------------------------------
def _round_up(n, block):
    return n if block == 0 else -(-n // block) * block


def _il_bits(il, bits):
    if il is None:
        return bits
    if il[0] == "block":
        return _round_up(bits, il[1] * il[2])
    return (_round_up(-(-bits // 8), il[1]) + il[1] * (il[1] - 1) * il[2]) * 8


def _bch_n(t):
    return BCH_INFO_BITS + len(RB.generator(t)) - 1


def block_plan(info_bytes, sch):
    """(info_bytes, framed_bytes, outer_coded_bits, outer_il_bits, inner_coded_bits, coded_bits)"""
    framed = info_bytes + CRC_LEN[sch["crc"]]
    outer, inner = sch["outer"], sch["inner"]
    if outer is None:
        oc = framed * 8
    elif outer[0] == "bch":
        oc = -(-framed * 8 // BCH_INFO_BITS) * _bch_n(outer[1])
    else:
        oc = -(-framed // (outer[1] - outer[2])) * outer[1] * 8
    oil = _il_bits(sch["outer_interleaver"], oc)
    if inner is None:
        ic = oil
    elif inner[0] == "ldpc":
        g = RL.graph(inner[1])
        ic = -(-oil // g.k) * g.n
    else:
        ic = RF.punctured_coded_len(inner[2], oil, inner[1])
    return info_bytes, framed, oc, oil, ic, _il_bits(sch["inner_interleaver"], ic)


# ---- encode_chain, ofdm_frame.rs:445-646 ----------------------------------------------------
def interleave_bits(il, bits):
    if il is None:
        return np.asarray(bits, np.uint8).copy()
    if il[0] == "block":
        return RF.interleave_bits(il[1], il[2], bits)
    return RR.bytes_to_bits(RR.frame_interleave(pack_bits_padded(bits), il[1], il[2]))


def _chunks(x, k):
    """x in rows of k, the last zero-padded."""
    x = np.asarray(x, np.uint8)
    rows = -(-len(x) // k)
    out = np.zeros((rows, k), np.uint8)
    out.reshape(-1)[:len(x)] = x
    return out


def outer_encode(outer, message):
    if outer is None:
        return RR.bytes_to_bits(message)
    if outer[0] == "bch":
        blocks = _chunks(RR.bytes_to_bits(message), BCH_INFO_BITS)
        return RB.encode(_bch_n(outer[1]), outer[1], blocks).reshape(-1) if len(blocks) else np.zeros(0, np.uint8)
    n, npar = outer[1], outer[2]
    words = [RR.rs_encode(n, npar, row) for row in _chunks(message, n - npar)]
    return RR.bytes_to_bits(np.concatenate(words)) if words else np.zeros(0, np.uint8)


def inner_encode(inner, bits):
    if inner is None:
        return np.asarray(bits, np.uint8).copy()
    if inner[0] == "ldpc":
        g = RL.graph(inner[1])
        blocks = _chunks(bits, g.k)
        return g.encode(blocks).reshape(-1) if len(blocks) else np.zeros(0, np.uint8)
    return np.asarray(RF.conv_encode_punctured(inner[2], bits, inner[1]), np.uint8)


def encode_chain_stages(data, sch, per_frame_seed=0):
    """(outer_il_bits, coded)"""
    framed = append_crc(sch["crc"], data)
    if sch["scrambler_pos"] == "before_outer":
        framed = scramble_bytes(sch, per_frame_seed, framed)
    outer_il = interleave_bits(sch["outer_interleaver"], outer_encode(sch["outer"], framed))
    coded = interleave_bits(sch["inner_interleaver"], inner_encode(sch["inner"], outer_il))
    s = build_scrambler(sch, per_frame_seed)
    if sch["scrambler_pos"] == "after_inner" and s:
        coded = scramble_bits(s, coded)
    return outer_il, coded


def encode_chain(data, sch, per_frame_seed=0):
    return encode_chain_stages(data, sch, per_frame_seed)[1]


# ---- decode_chain, demodulate/ofdm_frame.rs:351-725 -----------------------------------------
def deinterleave_bits(il, bits):
    bits = np.asarray(bits, np.uint8)
    if il is None:
        return bits.copy()
    if il[0] == "block":
        block = il[1] * il[2]
        out = [bits[at:at + block].copy() if len(bits) - at < block else RF.deinterleave(il[1], il[2], bits[at:at + block])
               for at in range(0, len(bits), block)]
        return np.concatenate(out) if out else bits.copy()
    total = len(bits) // 8
    d = il[1] * (il[1] - 1) * il[2]
    if total <= d:
        return np.zeros(0, np.uint8)
    return RR.bytes_to_bits(RR.frame_deinterleave(RR.bits_to_bytes(bits[:total * 8]), il[1], il[2])[:total - d])


def decode_chain(llr, plan, sch, per_frame_seed=0, ldpc_rule="sum_product"):
    """A dict of ChainOutcome's fields plus valid, or MALFORMED_HEADER."""
    _, framed_bytes, oc, oil, ic, coded_bits = plan
    llr = np.asarray(llr, np.float32)[:coded_bits].copy()
    s = build_scrambler(sch, per_frame_seed)
    if sch["scrambler_pos"] == "after_inner" and s:
        llr = apply_pn_to_llrs(s, llr)
    il = sch["inner_interleaver"]
    if il is not None and il[0] == "block":
        llr = RF.deinterleave_llrs(il[1], il[2], llr)
    llr = llr[:ic]
    inner, outer = sch["inner"], sch["outer"]
    inner_ok = True
    if inner is None:
        inner_out = (llr <= 0).astype(np.uint8)
    elif inner[0] == "ldpc":
        g = RL.graph(inner[1])
        nb = len(llr) // g.n
        inner_ok = len(llr) % g.n == 0
        if nb:
            bits, unsat, _, _ = RL.decode(inner[1], llr[:nb * g.n].reshape(nb, g.n), 50, ldpc_rule)
            inner_out, inner_ok = bits.reshape(-1), inner_ok and not unsat.any()
        else:
            inner_out = np.zeros(0, np.uint8)
    else:
        inner_out = np.asarray(RF.viterbi_decode_soft(inner[2], llr, oil, inner[1]), np.uint8)
    outer_de = deinterleave_bits(sch["outer_interleaver"], inner_out[:oil])[:oc]
    outer_ok, corrected = True, None
    if outer is None:
        framed_bits = outer_de
    elif outer[0] == "bch":
        n = _bch_n(outer[1])
        nb = len(outer_de) // n
        outer_ok = len(outer_de) % n == 0
        if nb:
            msgs, status, _ = RB.decode(n, outer[1], outer_de[:nb * n].reshape(nb, n))
            framed_bits, outer_ok = msgs.reshape(-1), outer_ok and not (status < 0).any()
        else:
            framed_bits = np.zeros(0, np.uint8)
    else:
        n, npar = outer[1], outer[2]
        coded_bytes = RR.bits_to_bytes(outer_de)
        outer_ok = len(coded_bytes) % n == 0
        corrected, msgs = 0, []
        for w in range(len(coded_bytes) // n):
            msg, count, _ = RR.rs_decode(n, npar, coded_bytes[w * n:(w + 1) * n])
            msgs.append(msg)
            if count < 0:
                outer_ok = False
            else:
                corrected += count
        framed_bits = RR.bytes_to_bits(np.concatenate(msgs)) if msgs else np.zeros(0, np.uint8)
    framed_bits = framed_bits[:framed_bytes * 8]
    if len(framed_bits) < framed_bytes * 8:
        return MALFORMED_HEADER
    framed = RR.bits_to_bytes(framed_bits)
    if sch["scrambler_pos"] == "before_outer":
        framed = scramble_bytes(sch, per_frame_seed, framed)
    stripped = check_and_strip_crc(sch["crc"], framed)
    if stripped is None:
        return MALFORMED_HEADER
    out = dict(bytes=stripped[0], inner_ok=bool(inner_ok), outer_ok=bool(outer_ok), crc_ok=bool(stripped[1]),
               crc_present=sch["crc"] != "none", outer_present=outer is not None, outer_corrected_bytes=corrected,
               inner_out_bits=inner_out)
    out["valid"] = out["crc_ok"] if out["crc_present"] else out["outer_ok"] if out["outer_present"] else out["inner_ok"]
    return out


# ---- the configurations and inputs the CPU and GPU tests share ------------------------------
LDPC_BCH = dict(outer=("bch", 8), inner=("ldpc", "n512r12"))           # the default ladder's chain
CONV_RS = dict(outer=("rs", 60, 8), inner=("conv", "1/2", "k5"))        # the reference's second workload
DVB = dict(crc="none", outer=("rs", 204, 16), inner=("conv", "3/4", "dvb_k7"), outer_interleaver=("forney", 12, 17),
           scrambler="dvbt")
HEADER = dict(crc="crc16", inner=("ldpc", "n512r12"))                   # the frame header's fixed chain
ADDITIVE = [(0b1001, 7), (0b11, 15), (0x80200003, 32)]  # (taps, width); 0b1001 / 7 is the reference tests' own
SEEDS = [0, 1, 0x5A, 0xFFFFFFFF, 0x12345678, 0x80, 0x8000, 0x10000]


def payload(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def clean_llrs(coded, amp=4.0):
    return ((1.0 - 2.0 * (np.asarray(coded, np.float32) % 2)) * np.float32(amp)).astype(np.float32)


def noisy_llrs(coded, sigma, seed):
    """BPSK over AWGN from a seeded generator: LLR = 2 y / sigma^2, in f32."""
    x = 1.0 - 2.0 * (np.asarray(coded, np.float64) % 2)
    y = x + np.random.default_rng(seed).normal(0.0, sigma, len(x))
    return (2.0 * y / sigma ** 2).astype(np.float32)


# The noisy set: AWGN on the coded bits of 24 frames of the default ladder's chain, at a level
# where (tests/test_frame_oracle.py asserts it under the host decoder alone) one frame fails its
# CRC, others pass although the inner decoder did not converge, and others are clean.
NOISY_SIGMA, NOISY_FRAMES = 0.8, 24


@functools.lru_cache(maxsize=None)
def noisy_set():
    """(sent (24, 96) uint8, llr (24, 3072) float32) under LDPC_BCH; leave them unchanged."""
    sch = scheme(**LDPC_BCH)
    sent = np.stack([payload(96, 100 + k) for k in range(NOISY_FRAMES)])
    llr = np.stack([noisy_llrs(encode_chain(sent[k], sch), NOISY_SIGMA, 1000 + k) for k in range(NOISY_FRAMES)])
    sent.flags.writeable = llr.flags.writeable = False
    return sent, llr


# ---- the frame layer at a known start: preamble, OfdmFrameMod::modulate_frame and
# OfdmFrameDemod::decode (sync/ofdm_sync.rs:142-352, modulate/ofdm_frame.rs:867-987,
# demodulate/ofdm_frame.rs:55-94, 862-1255), over np_ref_ofdm ----------------------------------
import np_ref_ofdm as RO  # noqa: E402

F = np.float32
HEADER_SCHEME_KEYS = dict(inner=("ldpc", "n512r12"))
RX = {"malformed_header": 2, "header_crc_mismatch": 3, "crc_mismatch": 4}


class Link:
    """A frame link: the plan (n_fft, cp_len, data carrier indices, no pilots), gain, window
    roll-off, the frame fields with the reference's defaults, the MCS table as (constellation,
    inner, outer) triples and the preamble (num_repeats, repeat_len, training or None)."""

    def __init__(self, n_fft, cp_len, data, gain=1.0, roll_off=0, mcs=None, preamble=(2, 32), training=True, **frame):
        self.n_fft, self.cp_len, self.data, self.gain, self.roll_off = n_fft, cp_len, np.asarray(data, np.int32), gain, roll_off
        self.mcs = mcs or [(c, ("ldpc", "n512r12"), ("bch", 8)) for c in ("bpsk", "qpsk", "qam16", "qam64")]
        self.preamble, self.training = preamble, (n_fft, cp_len) if training else None
        self.frame = dict(payload_crc="crc32", header_crc="crc16", outer_interleaver=None, inner_interleaver=None,
                          scrambler=None, scrambler_pos="before_outer", ldpc_decode_rule="sum_product")
        self.frame.update(frame)
        self.sps = n_fft + cp_len

    def symcfg(self, order):  # symbol_config: no window here, the post-pass tapers once
        z = np.zeros(0, np.int32)
        return RO.Config(self.n_fft, self.cp_len, self.data, z, np.zeros(0, np.complex64), gain=self.gain, order=order)

    def header_scheme(self):
        return scheme(crc=self.frame["header_crc"], **HEADER_SCHEME_KEYS)

    def payload_scheme(self, m):
        f = self.frame
        return scheme(crc=f["payload_crc"], outer=m[2], inner=m[1], outer_interleaver=f["outer_interleaver"],
                      inner_interleaver=f["inner_interleaver"], scrambler=f["scrambler"], scrambler_pos=f["scrambler_pos"])

    def symbols(self, order, bits):
        return -(-bits // (len(self.data) * RO.BITS[order]))


def unit_sequence(n, seed):  # ofdm_sync.rs:335-352
    state, mask, out = seed, (1 << 64) - 1, np.zeros(n, np.complex64)
    for i in range(2 * n):
        state ^= (state << 13) & mask
        state ^= state >> 7
        state ^= (state << 17) & mask
        v = F(F(np.uint64(state)) / F(2.0 ** 64)) - F(0.5)
        part = RO.FRAC_1_SQRT_2 if v >= 0 else -RO.FRAC_1_SQRT_2
        out[i // 2] += part if i % 2 == 0 else 1j * part
    return out


def preamble(link):  # generate_ofdm_preamble
    num, rl = link.preamble
    n_fft, z = link.n_fft, np.zeros(0, np.int32)
    half, base = RO.occupied_half_carriers(link.data, z), None
    if rl and n_fft % rl == 0 and half:
        k = n_fft // rl
        loaded = [b for i in range(1, half + 1) if i % k == 0 for b in (i, n_fft - i)]
        if loaded:
            freq = np.zeros(n_fft, np.complex64)
            freq[loaded] = unit_sequence(len(loaded), 0x4F46444D50524531)
            t = RO.fft_radix2(freq[None], True)[0][:rl]
            acc = F(0)
            for c in t:
                acc = F(acc + F(F(c.real * c.real) + F(c.imag * c.imag)))
            rms = np.sqrt(F(acc / F(rl)))
            if rms > 0:
                t = RO.gain(t, F(F(F(2.0) * np.sqrt(F(len(link.data)))) / F(n_fft)) / rms)
            base = t
    if base is None:
        base = unit_sequence(rl, 0x4F46444D50524531)
    parts = [base] * num
    if link.training:
        tn, tcp = link.training
        freq = RO.training_pattern(tn)
        occ = RO.occupied_bins(n_fft, link.data, z)
        keep = np.zeros(tn, bool)
        keep[occ[occ < tn]] = True
        freq = np.where(keep, freq, 0).astype(np.complex64)
        t = RO.fft_radix2(freq[None], True)[0]
        parts.append(np.concatenate([t[tn - tcp:], t]) if tcp else t)
    out = np.concatenate(parts).astype(np.complex64)
    return RO.gain(out, link.gain) if F(link.gain) != F(1.0) else out


def modulate_frame(link, mcs_index, sequence_num, flags, data, per_frame_seed=0):
    m = link.mcs[mcs_index]
    fields = pack_header_fields(mcs_index, len(data), sequence_num, flags, per_frame_seed)
    hdr = RO.modulate(link.symcfg("bpsk"), encode_chain(fields, link.header_scheme(), 0))
    pay = RO.modulate(link.symcfg(m[0]), encode_chain(data, link.payload_scheme(m), per_frame_seed))
    out = np.concatenate([preamble(link), hdr, pay]).astype(np.complex64)
    if link.roll_off:  # apply_symbol_windowing: whole symbols from the end of the raw repeats on
        start = link.preamble[0] * link.preamble[1]
        k = (len(out) - start) // link.sps
        body = out[start:start + k * link.sps].reshape(k, link.sps)
        out[start:start + k * link.sps] = RO.window_apply(body, RO.window_ramp(link.sps, link.roll_off)).reshape(-1)
    return out


def soft_demap(link, order, iq, n_sym):
    if len(iq) < n_sym * link.sps:
        return None
    return RO.soft_llr(order, RO.demodulate(link.symcfg(order), iq[:n_sym * link.sps]))


def decode_frame(link, iq):
    """(mcs_index, sequence_num, flags, payload) or the RxError code."""
    hs = link.header_scheme()
    hplan = block_plan(HEADER_FIELD_BYTES, hs)
    n_sym = link.symbols("bpsk", hplan[5])
    llr = soft_demap(link, "bpsk", iq, n_sym)
    if llr is None:
        return RX["malformed_header"]
    h = decode_chain(llr, hplan, hs, 0, "sum_product")
    if isinstance(h, int):
        return h
    if not h["valid"]:
        return RX["header_crc_mismatch"]
    b = bytes(h["bytes"])
    mcs_index, plen, seq, flags, seed = b[0], int.from_bytes(b[1:5], "big"), int.from_bytes(b[5:9], "big"), b[9], \
        int.from_bytes(b[10:14], "big")
    if mcs_index >= len(link.mcs):
        return RX["malformed_header"]
    m = link.mcs[mcs_index]
    ps = link.payload_scheme(m)
    plan = block_plan(plen, ps)
    llr = soft_demap(link, m[0], iq[n_sym * link.sps:], link.symbols(m[0], plan[5]))
    if llr is None:
        return RX["malformed_header"]
    out = decode_chain(llr, plan, ps, seed, link.frame["ldpc_decode_rule"])
    if isinstance(out, int):
        return out
    if not out["valid"]:
        return RX["crc_mismatch"]
    return mcs_index, seq, flags, out["bytes"][:plen]


def awgn(iq, sigma, seed):
    """Complex AWGN of standard deviation sigma per part from a seeded generator, in f32."""
    rng = np.random.default_rng(seed)
    n = (rng.standard_normal(len(iq)) + 1j * rng.standard_normal(len(iq))) * sigma
    return (np.asarray(iq, np.complex64) + n.astype(np.complex64)).astype(np.complex64)


# ---- the links and the noisy frame set the CPU and GPU frame-layer tests share ---------------
DATA62 = np.array([i for i in range(-31, 32) if i != 0], np.int32)  # n_fft 64: 62 data carriers, no pilots
CONV_RS_TABLE = [("qpsk", ("conv", "1/2", "k5"), ("rs", 60, 8))]
DVB_TABLE = [("qam16", ("conv", "3/4", "dvb_k7"), ("rs", 204, 16))]
DVB_FRAME = dict(payload_crc="none", outer_interleaver=("forney", 12, 17), scrambler="dvbt")
LEAD = 136  # two repeats of 32 and the training symbol of 64 + 8
FRAME_SIGMA, FRAME_COUNT = 0.07, 24


@functools.lru_cache(maxsize=None)
def noisy_frame_set():
    """(sent (24, 96) uint8, rx (24, 2448) complex64): frames of the default ladder's QPSK entry
    from the first sample after the training symbol, AWGN on the body at a level where
    (tests/test_frame_layer_oracle.py asserts it under the host decoder alone) some fail their
    payload CRC, some pass with an inner block that did not converge and some are clean."""
    link = Link(64, 8, DATA62)
    sent = np.stack([payload(96, 100 + k) for k in range(FRAME_COUNT)])
    rx = np.stack([awgn(modulate_frame(link, 1, k, k % 7, sent[k])[LEAD:], FRAME_SIGMA, 2000 + k) for k in range(FRAME_COUNT)])
    sent.flags.writeable = rx.flags.writeable = False
    return sent, rx
