#!/usr/bin/env python3
"""A long clip sampled whole against the same clip sampled in chunks with pinned overlap frames, on the GPU.

    python tools/bench_chunked.py [--frames 200] [--res 256] [--steps 50] [--chunk 56] [--overlap 8] [--reps 3] [--python-host]
                                  [--out FILE.json] [--commit TEXT]

Three numbers at the benchmark shape (256x256 -> 64x64 latent, 50 DDIM steps, dynamic thresholding, seeded noise, the C evaluator):
  whole        GaussianDiffusion.sample of the whole clip: nothing leaves the sampler before all of it is done, so this is also the time
               to its first frame;
  chunked      GaussianDiffusion.sample_chunked of the same clip (sampler.chunk_plan(frames, chunk, overlap)): slower in total, because
               the overlap frames are evaluated twice and a short chunk fills the deep levels worse;
  first chunk  from the call of iter_chunks to the first chunk's latent being complete on the device: the time to the first frame.
Device events around each run, ending in a synchronise; both forms are warmed up at their own shapes first (two steps each: code
objects, workspaces, allocator), then timed alternating, best of `--reps`.

What this does NOT measure: quality.  Whether a seam shows, whether the motion drifts over the chunks and which overlap is enough on a
trained checkpoint has not been measured by anyone; the weights here are random."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import UNET_KW  # noqa: E402
import dawn_pytorch_amd as D  # noqa: E402
from dawn_pytorch_amd.sampler import chunk_plan  # noqa: E402


def timed(fn):
    """milliseconds of fn() on the device: events around it, the second one synchronised."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def commit_text():
    try:
        r = subprocess.run(["git", "-C", ROOT, "describe", "--always", "--dirty"], capture_output=True, text=True, timeout=10)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown (not a git checkout)"
    except (OSError, subprocess.SubprocessError):
        return "unknown (git not available)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=56)
    ap.add_argument("--overlap", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--python-host", action="store_true", help="the Python orchestration instead of the C evaluator")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="what to name as the code that ran (default: git describe --always --dirty)")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if not torch.cuda.is_available():
        sys.exit("bench_chunked.py measures on the GPU; there is no CPU fallback")
    dev = torch.device("cuda:0")
    T, h = a.frames, a.res // 4
    plan = chunk_plan(T, a.chunk, a.overlap)
    unet = D.DynamicNfUnet3D(default_num_frames=T, num_frames=T, init_seed=0, **UNET_KW).to(dev)
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=unet, num_frames=T, image_size=h, sampling_timesteps=a.steps,
                                        timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                        ddim_sampling_eta=1.0).to(dev)
    diff.noise_seed, diff.use_ctx = 7, not a.python_host
    g = torch.Generator().manual_seed(123)
    fea = torch.randn(1, 256, h, h, generator=g).to(dev)
    bbox = torch.randn(1, 16, h, h, generator=g).to(dev)
    cond = torch.randn(1, T, 1032, generator=g).to(dev)

    def whole():
        return diff.sample(fea, bbox, cond=cond)

    def chunked():
        return diff.sample_chunked(fea, bbox, cond, 1.0, chunk_frames=a.chunk, overlap=a.overlap)

    def first_chunk():
        it = diff.iter_chunks(fea, bbox, cond, 1.0, chunk_frames=a.chunk, overlap=a.overlap)
        first = next(it)
        it.close()
        return first

    diff.sampling_timesteps = 2                      # warm-up at both shapes
    whole(), chunked()
    diff.sampling_timesteps = a.steps
    t_whole = t_chunked = t_first = float("inf")
    for _ in range(a.reps):
        t_whole = min(t_whole, timed(whole))
        t_chunked = min(t_chunked, timed(chunked))
        t_first = min(t_first, timed(first_chunk))
    evaluated = sum(n for _, n, _ in plan)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or commit_text(), "host": "python" if a.python_host else "ctx",
           "frames": T, "res": a.res, "latent": h, "steps": a.steps, "chunk": a.chunk, "overlap": a.overlap,
           "plan": [[s, n, kn] for s, n, kn in plan], "frames_evaluated": evaluated, "reps": a.reps,
           "whole_ms": round(t_whole, 1), "chunked_ms": round(t_chunked, 1), "first_chunk_ms": round(t_first, 1),
           "chunked_over_whole": round(t_chunked / t_whole, 3), "first_chunk_over_whole": round(t_first / t_whole, 3)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
