"""Writes tests/golden/small_lm_bits.npz: the outputs of every case of tests/test_gpu_small_lm_bits.py, recorded on the
GPU.  python tests/golden/make_small_lm_bits.py [output.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

import test_gpu_small_lm_bits as T  # noqa: E402

out = {}
for name, run in T.RUNS.items():
    got = run()
    out.update(got)
    print(name, len(got), "arrays", flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
