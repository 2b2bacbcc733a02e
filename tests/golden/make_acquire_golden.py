"""Writes tests/golden/acquire_golden.npz from the numpy restatement (tests/np_ref_acquire.py): one
capture of the acquisition tests (the default ladder's QPSK entry, 40 payload bytes, at offset 5
with a carrier offset of -28300 Hz, phase 2.0 rad and noise of 0.004 per part, over n_fft 64, cp
8, 62 data carriers, preamble 2 x 32 with a training symbol), the first 16 results of ofdm_sync
over it, and what the burst receiver makes of it: the payload's equalized symbols after the phase
tracker, the payload, consume_to, the start and the total carrier offset.
Run from the repository root: python tests/golden/make_acquire_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import np_ref_acquire as A  # noqa: E402
import np_ref_frame as R  # noqa: E402

link = R.Link(64, 8, R.DATA62)
data = R.payload(40, 43)
frame = R.modulate_frame(link, 1, 3, 3, data, 3)
total = 300 + len(R.modulate_frame(link, 0, 0, 0, R.payload(40, 0), 0))
x = A.impair(frame, 5, -28300.0, 2.0, A.SIGMA, 503, total=total)
res = A.ofdm_sync(x, 1e6, (2, 32, (64, 8)), 0, len(x))[:16]
step = A.receive(link, x)
assert step["error"] == 0 and np.array_equal(step["payload"], data)
np.savez_compressed(os.path.join(HERE, "acquire_golden.npz"), capture=x,
                    starts=np.array([r[0] for r in res], np.int64), cfo_hz=np.array([r[1] for r in res], np.float32),
                    bins=np.array([r[2] for r in res], np.int64), score=np.array([r[3] for r in res], np.float32),
                    symbols=np.asarray(step["symbols"], np.complex64), payload=step["payload"],
                    step=np.array([step["consume_to"], step["start_sample"]], np.int64),
                    cfo_total=np.array([step["cfo_hz"]], np.float32))
