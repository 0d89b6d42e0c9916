"""Records ``tt_step_bits.npz``: what tests/test_gpu_tt_step.py::step_bits gives for each of its shapes, on the GPU, with the
library built from the commit BEFORE a change of the seven-channel step's host code::

    QC_LIB=<libqcpinn_hip.so of that commit> python tests/golden/make_tt_step_bits.py

(without QC_LIB: the library of this tree).  Every shape runs twice, and once more with its first step issued as one call per
phase; the recording stops unless all three agree in every bit (the step's reductions are fixed-order).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_gpu_tt_step as T                 # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    out = {}
    for shape in T.BITS_SHAPES:
        a, b, c = T.step_bits(dev, *shape), T.step_bits(dev, *shape), T.step_bits(dev, *shape, split_first=True)
        for k, v in a.items():
            for other, what in ((b, "a second run"), (c, "one call per phase")):
                if not np.array_equal(v.view(np.uint32), other[k].view(np.uint32)):
                    sys.exit(f"{shape} {k}: {what} differs, max |difference| {np.abs(v - other[k]).max()}")
            assert np.isfinite(v).all()
            out["x".join(map(str, shape)) + "__" + k] = v
        print(shape, "loss sums per step", a["loss"].tolist())
    dst = os.environ.get("QC_BITS_OUT") or os.path.join(HERE, "tt_step_bits.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst)


if __name__ == "__main__":
    main()
