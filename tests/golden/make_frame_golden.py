"""Writes tests/golden/frame_golden.npz from the numpy restatement (tests/np_ref_frame.py): for
the three concatenations of the frame tests, three 96-byte payloads and their coded bits
(packed MSB first) under seed 0. Run from the repository root: python tests/golden/make_frame_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import np_ref_frame as R  # noqa: E402

out = {}
for name, kw in (("ldpc_bch", R.LDPC_BCH), ("conv_rs", R.CONV_RS), ("dvb", R.DVB)):
    sch = R.scheme(**kw)
    data = np.stack([R.payload(96, 40 + k) for k in range(3)])
    out[name + "_bytes"] = data
    out[name + "_coded"] = np.stack([np.packbits(R.encode_chain(d, sch, 0)) for d in data])
np.savez_compressed(os.path.join(HERE, "frame_golden.npz"), **out)
