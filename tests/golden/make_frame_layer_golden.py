"""Writes tests/golden/frame_layer_golden.npz from the numpy restatement (tests/np_ref_frame.py):
two 96-byte frames' bytes and IQ for the default ladder's QPSK entry with a window roll-off of 2,
and for convolutional K5 r1/2 + RS(60,52), over n_fft 64, cp 8, 62 data carriers, sequence number
and seed k. Run from the repository root: python tests/golden/make_frame_layer_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import np_ref_frame as R  # noqa: E402

out = {}
for name, link, mi in (("ldpc_bch", R.Link(64, 8, R.DATA62, roll_off=2), 1),
                       ("conv_rs", R.Link(64, 8, R.DATA62, mcs=R.CONV_RS_TABLE), 0)):
    data = np.stack([R.payload(96, 60 + k) for k in range(2)])
    out[name + "_bytes"] = data
    out[name + "_iq"] = np.stack([R.modulate_frame(link, mi, k, 0, data[k], k) for k in range(2)])
np.savez_compressed(os.path.join(HERE, "frame_layer_golden.npz"), **out)
