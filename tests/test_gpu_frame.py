"""GPU: the frame chain's glue kernels (csrc/k_frame.hip) and the batched chain wired from them
and the batched codes, against the library's host layer (csrc/frame.cpp, itself held to
tests/np_ref_frame.py by tests/test_frame_oracle.py). Everything is compared for equality, LLRs
as uint32: pack and unpack alone at every chunk geometry, frame count, CRC and whitener; the PN
on coded bits and on LLR rows; frame_encode_chain_batch against encode_chain and
frame_decode_chain_batch against decode_chain per frame in every returned field; torch tensors
on a stream of the caller's."""
import itertools

import numpy as np
import pytest

import np_ref_frame as R

pytestmark = pytest.mark.gpu
WAVES = 4  # frames per workgroup of k_frame_*

# fewer bytes than lanes, one per lane, one over, ragged chunks
INFO_LENS = [1, 14, 63, 64, 65, 96, 259, 1000]
WHITENERS = [None, "dvbt"] + [("additive", t, w, sd) for (t, w) in R.ADDITIVE for sd in (0x2B, "per_frame")]


def seeds_for(nframes, salt):
    """Distinct per frame, the special ones first: 0 (mapped to 1), all ones, a high bit alone."""
    s = np.array([(R.SEEDS[(k + salt) % len(R.SEEDS)] + 0x01010101 * (k // len(R.SEEDS))) & 0xFFFFFFFF
                  for k in range(nframes)], np.int64)
    return s


def host_pack(lib, sch, payloads, seeds):
    return np.stack([lib.scramble_bytes(sch, lib.append_crc(sch.crc, p), int(s)) for p, s in zip(payloads, seeds)])


@pytest.mark.parametrize("info_len", INFO_LENS)
def test_pack_and_unpack_alone(gpu_lib, info_len):
    lib = gpu_lib
    combo = 0
    for crc, wh, nframes in itertools.product(("none", "crc16", "crc32"), WHITENERS, (1, WAVES, WAVES + 1)):
        combo += 1
        sch = lib.FrameScheme(crc=crc, scrambler=wh)
        rng = np.random.default_rng([info_len, combo])
        payloads = rng.integers(0, 256, (nframes, info_len), dtype=np.uint8)
        seeds = seeds_for(nframes, combo)
        want = host_pack(lib, sch, payloads, seeds)
        arg = seeds if sch.per_frame_seed else None
        got_bytes = lib.frame_pack_batch(payloads, sch, seeds=arg, out_bytes=True)
        assert got_bytes.dtype == np.uint8 and np.array_equal(got_bytes, want), (crc, wh, nframes)
        got_bits = lib.frame_pack_batch(payloads, sch, seeds=arg)
        assert np.array_equal(got_bits, np.unpackbits(want, axis=1)), (crc, wh, nframes)

        # unpack: rows wider than the block, element values other than 0 and 1, one flipped bit
        bits = np.concatenate([got_bits | 0xFE, np.full((nframes, 13), 1, np.uint8)], axis=1)
        hit = nframes - 1
        at = int(rng.integers(0, got_bits.shape[1]))
        bits[hit, at] ^= 1
        broken = want.copy()
        broken[hit, at // 8] ^= 0x80 >> (at % 8)
        unsat = (rng.integers(0, 2, (nframes, 6)) * (np.arange(nframes)[:, None] % 2)).astype(np.int32)
        status = rng.integers(-1, 4, (nframes, 7)).astype(np.int32)
        status[0] = abs(status[0])
        for x, in_bytes in ((bits, False), (np.concatenate([broken, broken[:, :3]], axis=1), True)):
            out = lib.frame_unpack_batch(x, info_len, sch, seeds=arg, in_bytes=in_bytes, unsat=unsat, status=status)
            for k in range(nframes):
                pay, ok = lib.check_and_strip_crc(crc, lib.scramble_bytes(sch, broken[k], int(seeds[k])))
                assert np.array_equal(out["payload"][k], pay) and bool(out["crc_ok"][k]) == ok, (crc, wh, k)
                assert ok == (k != hit or crc == "none")
                assert np.array_equal(pay, payloads[k]) == (k != hit or at >= 8 * info_len)
            assert np.array_equal(out["inner_ok"], ~(unsat != 0).any(axis=1))
            assert np.array_equal(out["outer_ok"], ~(status < 0).any(axis=1))
            assert np.array_equal(out["corrected"], np.where(status > 0, status, 0).sum(axis=1))
            # no outer code in this scheme: the CRC decides, else the inner decoder
            assert np.array_equal(out["valid"], out["crc_ok"] if crc != "none" else out["inner_ok"])
        plain = lib.frame_unpack_batch(got_bits, info_len, sch, seeds=arg)
        assert np.array_equal(plain["payload"], payloads) and plain["crc_ok"].all() and plain["inner_ok"].all()
        assert plain["outer_ok"].all() and plain["valid"].all() and not plain["corrected"].any()


def test_unpack_validity_precedence_with_an_outer_code(gpu_lib):
    lib = gpu_lib
    payloads = np.stack([R.payload(40, k) for k in range(6)])
    status = np.array([[0, 0], [0, -1], [2, 3], [-4, 1], [0, 0], [1, 0]], np.int32)
    unsat = np.array([[0], [0], [3], [0], [1], [0]], np.int32)
    for crc in ("none", "crc32"):
        sch = lib.FrameScheme(crc=crc, outer=("rs", 60, 8), inner=("ldpc", "n512r12"))
        x = lib.frame_pack_batch(payloads, sch, out_bytes=True)
        x[5, 0] ^= 1
        out = lib.frame_unpack_batch(x, 40, sch, in_bytes=True, unsat=unsat, status=status)
        outer_ok = ~(status < 0).any(axis=1)
        assert np.array_equal(out["outer_ok"], outer_ok) and np.array_equal(out["inner_ok"], unsat[:, 0] == 0)
        assert np.array_equal(out["crc_ok"], np.arange(6) != 5 if crc != "none" else np.ones(6, bool))
        assert np.array_equal(out["valid"], out["crc_ok"] if crc != "none" else outer_ok)
        assert out["corrected"].tolist() == [0, 0, 5, 1, 0, 1]


@pytest.mark.parametrize("nframes", [1, WAVES, WAVES + 1])
def test_header_mode_returns_every_field(gpu_lib, nframes):
    lib = gpu_lib
    rng = np.random.default_rng(nframes)
    fields = np.stack([rng.integers(0, 256, nframes), rng.integers(0, 1 << 32, nframes), rng.integers(0, 1 << 32, nframes),
                       rng.integers(0, 256, nframes), rng.integers(0, 1 << 32, nframes)], axis=1).astype(np.int64)
    fields[0] = [255, 0xFFFFFFFF, 0x80000000, 255, 0xFFFFFFFF]
    for crc in ("crc16", "crc32", "none"):
        sch = lib.FrameScheme(crc=crc)
        want = np.stack([lib.append_crc(crc, lib.pack_header_fields(*(int(v) for v in f))) for f in fields])
        got = lib.frame_pack_batch(None, sch, fields=fields)
        assert np.array_equal(got, np.unpackbits(want, axis=1))
        out = lib.frame_unpack_batch(got, 14, sch, header=True)
        assert out["fields"].dtype == np.int64 and np.array_equal(out["fields"], fields) and out["crc_ok"].all()
        assert np.array_equal(out["payload"], want[:, :14])
        got[nframes - 1, 9] ^= 1  # bit 30 of payload_len: byte 1, second from the top
        out = lib.frame_unpack_batch(got, 14, sch, header=True)
        assert bool(out["crc_ok"][nframes - 1]) == (crc == "none")
        assert out["fields"][nframes - 1, 1] == fields[nframes - 1, 1] ^ (1 << 30)


@pytest.mark.parametrize("nbits,out_len,stride", [(1932, 1984, 1984), (3072, 3100, 3348), (5, 5, 8)])
@pytest.mark.parametrize("taps,width", R.ADDITIVE)
def test_pn_on_bits_and_on_llrs(gpu_lib, taps, width, nbits, out_len, stride):
    lib = gpu_lib
    nframes = WAVES + 1
    rng = np.random.default_rng([width, nbits])
    bits = rng.integers(0, 2, (nframes, stride), dtype=np.uint8)
    llr = rng.standard_normal((nframes, stride)).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, -np.nan], np.float32)
    llr[:, :8] = special[:min(8, stride)]
    llr[:, nbits - 4:nbits] = special[:4]
    seeds = seeds_for(nframes, width)
    for sd in (0x2B, "per_frame"):
        sch = lib.FrameScheme(scrambler=("additive", taps, width, sd), scrambler_pos="after_inner")
        arg = seeds if sd == "per_frame" else None
        got = lib.frame_coded_bits_batch(bits, sch, nbits=nbits, out_len=out_len, seeds=arg)
        got_l = lib.frame_llr_prepare_batch(llr, nbits, sch, seeds=arg)
        assert got.shape == (nframes, out_len) and got_l.shape == (nframes, nbits)
        for k in range(nframes):
            assert np.array_equal(got[k, :nbits], lib.scramble_bits(sch, bits[k, :nbits], int(seeds[k]))), (sd, k)
            assert not got[k, nbits:].any()
            want = lib.apply_pn_to_llrs(sch, llr[k, :nbits], int(seeds[k]))
            assert np.array_equal(got_l[k].view(np.uint32), want.view(np.uint32)), (sd, k)
    # a scrambler that sits elsewhere, or none: the rows are copied and padded
    for sch in (lib.FrameScheme(), lib.FrameScheme(scrambler=("additive", taps, width, 1)), lib.FrameScheme(scrambler="dvbt")):
        raw = bits | 0x10
        got = lib.frame_coded_bits_batch(raw, sch, nbits=nbits, out_len=out_len)
        assert np.array_equal(got[:, :nbits], raw[:, :nbits]) and not got[:, nbits:].any()
        got_l = lib.frame_llr_prepare_batch(llr, nbits, sch)
        assert np.array_equal(got_l.view(np.uint32), llr[:, :nbits].view(np.uint32))


def test_bytes_to_bits(gpu_lib):
    x = np.random.default_rng(9).integers(0, 256, (WAVES + 1, 61), dtype=np.uint8)
    assert np.array_equal(gpu_lib.frame_bytes_to_bits_batch(x), np.unpackbits(x, axis=1))


CHAINS = {
    "ldpc_bch": dict(R.LDPC_BCH),
    "conv_rs": dict(R.CONV_RS),
    "dvb": dict(R.DVB),
    "ldpc_bch_pn_after": dict(R.LDPC_BCH, scrambler=("additive", 0b1001, 7, "per_frame"), scrambler_pos="after_inner"),
    "k7_1932_pn_after": dict(outer=("rs", 60, 8), inner=("conv", "1/2", "dvb_k7"),
                             scrambler=("additive", 0b11, 15, "per_frame"), scrambler_pos="after_inner"),
    "conv_rs_pn_before_il": dict(R.CONV_RS, scrambler=("additive", 0x80200003, 32, "per_frame"),
                                 inner_interleaver=("block", 8, 31)),
    "ldpc_il_crc16": dict(crc="crc16", outer=("bch", 4), inner=("ldpc", "n576r23"), inner_interleaver=("block", 16, 40)),
    "bare": dict(crc="crc16"),
}


def same_fields(lib, out, k, want):
    assert np.array_equal(out["payload"][k], want.bytes), k
    assert (bool(out["inner_ok"][k]), bool(out["outer_ok"][k]), bool(out["crc_ok"][k]), bool(out["valid"][k])) == \
        (want.inner_ok, want.outer_ok, want.crc_ok, want.is_valid()), k
    assert np.array_equal(out["inner_out_bits"][k], want.inner_out_bits), k
    if want.outer_corrected_bytes is not None:
        assert int(out["corrected"][k]) == want.outer_corrected_bytes, k


@pytest.mark.parametrize("name", list(CHAINS))
def test_chain_batch_equals_the_host_chain_per_frame(gpu_lib, name):
    lib = gpu_lib
    sch = lib.FrameScheme(**CHAINS[name])
    for n, nframes in ((96, 3), (37, WAVES + 1)):
        payloads = np.stack([R.payload(n, 7 * k + n) for k in range(nframes)])
        seeds = seeds_for(nframes, n)
        arg = seeds if sch.per_frame_seed else None
        plan = lib.block_plan(n, sch)
        pad = plan.coded_bits + 45
        coded = lib.frame_encode_chain_batch(payloads, sch, seeds=arg, out_len=pad)
        assert coded.shape == (nframes, pad) and not coded[:, plan.coded_bits:].any()
        for k in range(nframes):
            assert np.array_equal(coded[k, :plan.coded_bits], lib.encode_chain(payloads[k], sch, int(seeds[k]))), k
        assert np.array_equal(lib.frame_encode_chain_batch(payloads, sch, seeds=arg), coded[:, :plan.coded_bits])
        # clean rows, noisy rows and rows wider than the block
        llr = np.stack([R.clean_llrs(coded[k, :plan.coded_bits]) if k % 2 == 0 else
                        R.noisy_llrs(coded[k, :plan.coded_bits], 0.85, k) for k in range(nframes)])
        wide = np.concatenate([llr, np.full((nframes, 45), -3.0, np.float32)], axis=1)
        for x in (llr, wide):
            out = lib.frame_decode_chain_batch(x, n, sch, seeds=arg)
            for k in range(nframes):
                same_fields(lib, out, k, lib.decode_chain(x[k], n, sch, int(seeds[k])))
            assert out["valid"][0] and np.array_equal(out["payload"][0], payloads[0])


def test_header_chain_batch(gpu_lib):
    lib = gpu_lib
    sch = lib.FrameScheme(**R.HEADER)
    fields = np.array([[1, 96, 7, 0, 0x12345678], [3, 1000, 0xFFFFFFFF, 255, 0], [0, 0, 0, 1, 1]], np.int64)
    coded = lib.frame_encode_chain_batch(None, sch, fields=fields, out_len=9 * 62)
    assert coded.shape == (3, 558)
    for k, f in enumerate(fields):
        want = lib.encode_chain(lib.pack_header_fields(*(int(v) for v in f)), sch)
        assert np.array_equal(coded[k, :512], want) and not coded[k, 512:].any()
    llr = np.stack([R.noisy_llrs(coded[k], 0.6, k) for k in range(3)])
    llr[2, :256] = -llr[2, :256]  # a header beyond repair
    out = lib.frame_decode_chain_batch(llr, 14, sch, header=True)
    for k in range(3):
        want = lib.decode_chain(llr[k], 14, sch)
        same_fields(lib, out, k, want)
        assert tuple(int(v) for v in out["fields"][k]) == lib.unpack_header_fields(want.bytes)
    assert out["valid"][:2].all() and np.array_equal(out["fields"][:2], fields[:2]) and not out["valid"][2]


def test_noisy_set_equals_the_host_decoder(gpu_lib):
    lib = gpu_lib
    sch = lib.FrameScheme(**R.LDPC_BCH)
    sent, llr = R.noisy_set()
    out = lib.frame_decode_chain_batch(llr, 96, sch)
    for k in range(len(llr)):
        same_fields(lib, out, k, lib.decode_chain(llr[k], 96, sch))
    ok = out["crc_ok"]
    assert (~ok).any() and (ok & ~out["inner_ok"]).any() and (ok & out["inner_ok"] & out["outer_ok"]).any()
    assert np.array_equal(ok, (out["payload"] == sent).all(axis=1))


def test_torch_tensors_on_a_stream_of_the_callers(gpu_lib):
    import torch

    lib = gpu_lib
    sch = lib.FrameScheme(**CHAINS["ldpc_bch_pn_after"])
    payloads = np.stack([R.payload(96, k) for k in range(WAVES + 1)])
    seeds = seeds_for(WAVES + 1, 3)
    want = lib.frame_encode_chain_batch(payloads, sch, seeds=seeds, out_len=3100)
    llr = np.stack([R.noisy_llrs(want[k], 0.75, k) for k in range(len(want))])
    want_out = lib.frame_decode_chain_batch(llr, 96, sch, seeds=seeds)
    s = torch.cuda.Stream()
    tp, ts, tl = torch.from_numpy(payloads).cuda(), torch.from_numpy(seeds).cuda(), torch.from_numpy(llr).cuda()
    torch.cuda.synchronize()
    # the stream is given by its handle alone: torch's own slices and pads inside the call follow it
    coded = lib.frame_encode_chain_batch(tp, sch, seeds=ts, out_len=3100, stream=s.cuda_stream)
    out = lib.frame_decode_chain_batch(tl, 96, sch, seeds=ts, stream=s.cuda_stream)
    s.synchronize()
    assert coded.is_cuda and coded.dtype == torch.uint8 and np.array_equal(coded.cpu().numpy(), want)
    for key in ("payload", "inner_ok", "outer_ok", "crc_ok", "valid", "corrected", "inner_out_bits"):
        assert out[key].is_cuda and np.array_equal(out[key].cpu().numpy(), want_out[key]), key
    out = lib.frame_decode_chain_batch(tl, 96, sch, seeds=seeds)  # host seeds, torch's current stream
    assert np.array_equal(out["payload"].cpu().numpy(), want_out["payload"])
    for bad in (lambda: lib.frame_pack_batch(torch.from_numpy(payloads), sch),  # a CPU tensor
                lambda: lib.frame_pack_batch(tp[:, ::2], sch),
                lambda: lib.frame_llr_prepare_batch(tl, 4000, sch, seeds=ts),
                lambda: lib.frame_coded_bits_batch(coded, sch),  # the per-frame seeds are missing
                lambda: lib.frame_unpack_batch(coded[:, :100].contiguous(), 96, sch)):
        with pytest.raises(ValueError):
            bad()


def test_what_the_batched_chain_does_not_take(gpu_lib):
    lib = gpu_lib
    p = np.zeros((2, 96), np.uint8)
    for kw in (dict(R.LDPC_BCH, outer_interleaver=("block", 8, 23)), dict(outer_interleaver=("forney", 4, 3), outer=("bch", 2)),
               dict(inner_interleaver=("block", 3, 11)), dict(R.LDPC_BCH, inner_interleaver=("forney", 4, 3))):
        sch = lib.FrameScheme(**kw)
        with pytest.raises(ValueError):
            lib.frame_encode_chain_batch(p, sch)
        with pytest.raises(ValueError):
            lib.frame_decode_chain_batch(np.zeros((2, lib.block_plan(96, sch).coded_bits), np.float32), 96, sch)
        assert lib.encode_chain(p[0], sch).size == lib.block_plan(96, sch).coded_bits  # the host chain does
    with pytest.raises(ValueError):
        lib.frame_pack_batch(np.zeros((1, (1 << 16) + 1), np.uint8), lib.FrameScheme())
    with pytest.raises(ValueError):
        lib.frame_decode_chain_batch(np.zeros((2, 3000), np.float32), 96, lib.FrameScheme(**R.LDPC_BCH))


@pytest.mark.parametrize("crc", ["crc16", "crc32"])
def test_an_empty_block_is_its_crc(gpu_lib, crc):
    lib = gpu_lib
    for wh in (None, ("additive", 0b1001, 7, "per_frame")):
        sch = lib.FrameScheme(crc=crc, scrambler=wh)
        seeds = seeds_for(WAVES + 1, 2)
        arg = seeds if wh else None
        got = lib.frame_pack_batch(np.zeros((WAVES + 1, 0), np.uint8), sch, seeds=arg, out_bytes=True)
        assert np.array_equal(got, host_pack(lib, sch, np.zeros((WAVES + 1, 0), np.uint8), seeds))
        out = lib.frame_unpack_batch(got, 0, sch, seeds=arg, in_bytes=True)
        assert out["payload"].shape == (WAVES + 1, 0) and out["crc_ok"].all() and out["valid"].all()
        got[1, 0] ^= 4
        assert lib.frame_unpack_batch(got, 0, sch, seeds=arg, in_bytes=True)["crc_ok"].tolist() == [True, False, True, True, True]
