#!/usr/bin/env python3
"""GPU box: the resampler to 16 kHz (csrc/audio_resample.hip) on 10 s of stereo PCM at 44.1 and 48 kHz, beside the HuBERT stage on the
16 kHz samples it makes, in one run.

    python tools/bench_audio_resample.py [--seconds 10] [--reps 50] [--warmup 5] [--layers 24] [--stage-reps 5] [--out FILE]
    python tools/bench_audio_resample.py --trace-loop 20 --rates 44100      the calls alone, for a kernel trace in a run of its own

  call   HipOps.resample_to_16k: HIP events around the call (the binding's Python overhead, the table launch and the FIR launch), warm,
         median / minimum / maximum over --reps.  The two launches apart are read off a kernel trace of --trace-loop
         (rocprofv3 --kernel-trace --stats, then tools/rocpd_summary.py): events cannot stand between two launches of one C call.
  stage  dawn_hubert_features (hubert-large widths, seeded random weights, tools/bench_hubert.py) on the resampled 10 s; host wall
         clock around a call that ends with the rows in host memory.

Prints one JSON line.  A report, not a gate; there is no CPU fallback (no GPU: an error)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEFAULT_RATES = (44100, 48000)


def stereo_pcm(rate, seconds, seed=0):
    n = int(rate * seconds)
    rng = np.random.default_rng(seed + rate)
    t = np.arange(n) / rate
    ch0 = 8000 * np.sin(2 * np.pi * 180 * t) + 4000 * np.sin(2 * np.pi * 2300 * t) + 1500 * rng.standard_normal(n)
    return torch.from_numpy(np.stack((ch0, 3000 * rng.standard_normal(n)), 1).astype(np.int16)).contiguous().cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--trace-loop", type=int, default=0, help="only run the call this many times per rate (for a kernel trace)")
    ap.add_argument("--rates", type=int, nargs="+", default=list(DEFAULT_RATES), help="input rates (a trace of one rate tells its launches apart)")
    ap.add_argument("--out", help="also write the JSON record to this file")
    args = ap.parse_args()
    RATES = tuple(args.rates)
    if not torch.cuda.is_available():
        sys.exit("bench_audio_resample: needs a GPU (a timing taken anywhere else says nothing about it)")
    from bench_hubert import CONV_STRIDE, event_ms, hubert_large_state_dict, wall_ms
    from dawn_pytorch_amd import _lib
    from dawn_pytorch_amd.ops import HipOps
    ops = HipOps()
    pcm = {rate: stereo_pcm(rate, args.seconds) for rate in RATES}
    if args.trace_loop:
        for rate in RATES:
            for _ in range(args.trace_loop):
                ops.resample_to_16k(pcm[rate], rate)
        torch.cuda.synchronize()
        return
    rec = {"device": torch.cuda.get_device_name(0), "seconds": args.seconds, "call": {}}
    samples = {}
    for rate in RATES:
        for _ in range(args.warmup):
            samples[rate] = ops.resample_to_16k(pcm[rate], rate)
        torch.cuda.synchronize()
        t = [event_ms(lambda: ops.resample_to_16k(pcm[rate], rate))[0] for _ in range(args.reps)]
        rec["call"][str(rate)] = {"frames_in": int(pcm[rate].shape[0]), "samples_out": int(samples[rate].numel()),
                                  "table_bytes": int(_lib.lib().dawn_resample16k_workspace_bytes(rate)),
                                  "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    from dawn_pytorch_amd.hubert import HubertFeatures
    hf = HubertFeatures(hubert_large_state_dict(args.layers), "cuda:0", num_heads=16, conv_stride=CONV_STRIDE, pos_groups=16)
    speech = samples[RATES[0]]
    for _ in range(2):
        rows = hf.process_audio(speech, via_c=True)
    t = [wall_ms(lambda: hf.process_audio(speech, via_c=True))[0] for _ in range(args.stage_reps)]
    rec["stage"] = {"layers": args.layers, "samples": int(speech.numel()), "rows_out": int(rows.shape[0]),
                    "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
    for rate in RATES:
        rec["call"][str(rate)]["share_of_stage"] = round(rec["call"][str(rate)]["median_ms"] / rec["stage"]["median_ms"], 5)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
