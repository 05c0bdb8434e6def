#!/usr/bin/env python3
"""Writes tests/golden/length_F{F}_h{h}.npz for every case of tests/length_cases.py: the float64 evaluation of the whole UNet by the
project's oracle (oracle/dawn_oracle.unet_forward on float64 weights and inputs) that tests/test_hip_length_gates.py holds the GPU
evaluation against, and the error of the same oracle in float32 on this CPU that scales the gate.  CPU only; a few minutes.

    python tools/gen_goldens_lengths.py [F{F}_h{h} ...]        (no argument: every case)

Each fixture holds
    y64                 float64 oracle output (3, kept frames, h, h)
    frames              the kept frame indices (length_cases.kept_frames)
    e32                 max|y32 - y64| / max|y64| on the kept frames (split_gate.rel_err), y32 = the oracle in float32 with oneDNN and NNPACK
                        off (torch's im2col + GEMM convolution, as split_gate.Case.base32); e32_all: the same over every frame
    threads, torch_version   of the run that measured e32 (a float32 sum depends on how the GEMM blocks it)
    inputs_checksum, weights_checksum, T, h, time     as the full_*.npz fixtures
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import length_cases as L          # noqa: E402


def main(argv):
    unet, wsum = L.full_unet()
    sd = dict(unet.state_dict())
    for F, h, t in L.CASES:
        if argv and L.case_name(F, h) not in argv:
            continue
        t0 = time.time()
        x, cond, isum = L.clip(F, h)
        y64 = L.oracle(sd, x, cond, t, torch.float64)
        y32 = L.oracle(sd, x, cond, t, torch.float32).double()
        fr = L.kept_frames(F, h)
        k64, k32 = y64[:, fr], y32[:, fr]
        path = os.path.join(ROOT, "tests", "golden", L.fixture_name(F, h))
        np.savez(path, y64=k64.numpy(), frames=np.asarray(fr, dtype=np.int64),
                 e32=np.float64((k32 - k64).abs().max() / k64.abs().max()), e32_all=np.float64((y32 - y64).abs().max() / y64.abs().max()),
                 threads=np.int64(torch.get_num_threads()), torch_version=np.asarray(torch.__version__),
                 inputs_checksum=isum, weights_checksum=wsum, T=np.int64(F), h=np.int64(h), time=np.int64(t))
        size = os.path.getsize(path)
        if size >= L.FIXTURE_LIMIT:
            raise SystemExit(f"{path}: {size} bytes")
        print(f"{L.case_name(F, h)}: {len(fr)} of {F} frames, {size} bytes, e32 {float((k32 - k64).abs().max() / k64.abs().max()):.3e}, "
              f"|y|max {float(k64.abs().max()):.3f}, {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
