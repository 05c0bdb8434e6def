#!/usr/bin/env python3
"""GPU box: how long a full-size model bundle takes to load (include/dawn_hip.h, "model bundle").

    python tools/bench_bundle.py [--dir DIR] [--reps 5] [--hubert-layers 24] [--out profiles/bundle_load.json]

Builds the full architecture with seeded random weights through the real packers -- HuBERT-large (24 layers, hidden 1024), the two
PBnets at the shipped widths, the LFG decoder, the face-location encoder and the 64-wide four-level UNet of bench.py -- writes it with
bundle.bundle_from_pipeline into DIR (a temporary directory unless given; the file is removed afterwards), then times, with a host clock
around calls that end in a stream synchronise:

  upload   dawn_bundle_upload of the whole device part, --reps times.  The file has just been written, so it is read from the page cache
           of the host, not from the medium: the figure is the loader's own ceiling (fread into two pinned 8 MiB buffers + the copies),
           and a cold read is bounded by the file system below that.  The file system of DIR is reported.
  verify   dawn_bundle_verify, one warm-up and --reps calls: work list to the device, the checksum launch, the partial pairs back, the
           per-tensor sums on the host.  bytes/s = device bytes over the call's wall time (an end-to-end rate, not a kernel's share of peak).
  create   dawn_bundle_create_handles, once.

Prints one JSON line and writes it to --out.  A report, not a gate; no GPU: an error."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def filesystem_of(path):
    """(mount point, type) of the longest mount prefix of `path`."""
    path, best = os.path.realpath(path), ("?", "?")
    try:
        for line in open("/proc/mounts"):
            _, mnt, kind = line.split()[:3]
            if (path == mnt or path.startswith(mnt.rstrip("/") + "/")) and len(mnt) >= len(best[0]):
                best = (mnt, kind)
    except OSError:
        pass
    return best


def full_pipeline(hubert_layers):
    import bench
    import bench_decode
    import bench_hubert
    import bench_pbnet
    from dawn_pytorch_amd import ctx
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.flow_diffusion import Face_loc_Encoder
    from dawn_pytorch_amd.hubert import HubertFeatures
    from dawn_pytorch_amd.ops import HipOps
    from dawn_pytorch_amd.pbnet import PoseBlinkGenerator
    ops = HipOps()
    hf = HubertFeatures(bench_hubert.hubert_large_state_dict(hubert_layers), "cuda:0", num_heads=16, conv_stride=bench_hubert.CONV_STRIDE,
                        pos_groups=16)
    gp = PoseBlinkGenerator(bench_pbnet.decoder_state_dict(6, seed=1), archiname="transformerreemb6", device="cuda", ops=ops)
    gb = PoseBlinkGenerator(bench_pbnet.decoder_state_dict(2, seed=2), archiname="transformerreemb5", device="cuda", ops=ops)
    dec = FlowDecoder(bench_decode.lfg_state_dict(0), "cuda", ops=ops)
    unet, _ = bench.build_model(200, 64, 20, "cuda:0")

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.face_loc_emb, self.pose_dim = Face_loc_Encoder(), 6
    fl = Holder().cuda()
    pipe = ctx.PipelineEvaluator(hf.evaluator(), gp.c_evaluator(), gb.c_evaluator(), ctx.DecoderEvaluator(dec),
                                 ctx.InputsEvaluator(fl, n_aud=1024), ctx.CtxEvaluator(unet.packed()))
    return pipe, (hf, gp, gb, dec, unet, fl)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hubert-layers", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_load.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bundle: needs a GPU (a timing taken anywhere else says nothing about it)")
    from dawn_pytorch_amd import _lib, bundle, ctx
    from dawn_pytorch_amd.sampler import ancestral_step_scalars, cosine_schedule_buffers, ddim_step_scalars
    L = _lib.lib()
    t0 = time.perf_counter()
    pipe, keep = full_pipeline(args.hubert_layers)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    bufs = cosine_schedule_buffers(1000)
    steps = {"ddim.20": ddim_step_scalars(bufs, 20, 1.0), "ddim.50": ddim_step_scalars(bufs, 50, 1.0)}
    if "posterior_mean_coef1" in bufs:
        steps["ancestral.1000"] = ancestral_step_scalars(bufs, 1000)
    tmp = tempfile.TemporaryDirectory(dir=args.dir)
    path = os.path.join(tmp.name, "full.dawn")
    t0 = time.perf_counter()
    idx = bundle.bundle_from_pipeline(path, pipe, steps)
    t_write = time.perf_counter() - t0
    per_stage = {}
    for e in idx["entries"]:
        if e["kind"] == 0:
            n, b = per_stage.get(e["stage"], (0, 0))
            per_stage[e["stage"]] = (n + 1, b + e["length"])
    del pipe, keep                                          # the evaluators' weights leave the device before the region arrives
    torch.cuda.empty_cache()

    b = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.dawn_bundle_open(path.encode(), C.addressof(b)), "dawn_bundle_open")
    t_open = time.perf_counter() - t0
    nbytes, need = int(L.dawn_bundle_device_bytes(b)), int(L.dawn_bundle_verify_workspace_bytes(b))
    mem = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    upload = lambda: _lib.check(L.dawn_bundle_upload(b, mem.data_ptr(), nbytes, stream), "dawn_bundle_upload")                  # noqa: E731
    verify = lambda: _lib.check(L.dawn_bundle_verify(b, mem.data_ptr(), nbytes, ws.data_ptr(), need, stream), "dawn_bundle_verify")  # noqa: E731
    t_upload = [timed(upload) for _ in range(args.reps)]
    timed(verify)                                            # warm-up: the code object loads on the first launch
    t_verify = [timed(verify) for _ in range(args.reps)]
    a = ctx.GenerateArgs()
    t_create = timed(lambda: _lib.check(L.dawn_bundle_create_handles(b, mem.data_ptr(), C.addressof(a)), "dawn_bundle_create_handles"))
    L.dawn_bundle_destroy_handles(C.addressof(a))
    L.dawn_bundle_close(b)
    mnt, kind = filesystem_of(tmp.name)
    med = statistics.median
    out = dict(device=torch.cuda.get_device_name(0), file_bytes=idx["file_bytes"], device_bytes=nbytes, entries=idx["n_entries"],
               tensors_and_bytes_per_stage=per_stage, verify_workspace_bytes=need, work_items=sum(-(-e["length"] // (4 * 65536)) for e in idx["entries"] if e["kind"] == 0),
               hubert_layers=args.hubert_layers, directory_mount=mnt, directory_filesystem=kind, page_cache="warm (the file was just written)",
               build_models_s=round(t_build, 3), write_s=round(t_write, 3), open_s=round(t_open, 4),
               upload_s=[round(t, 4) for t in t_upload], upload_median_s=round(med(t_upload), 4), upload_GBps=round(nbytes / med(t_upload) / 1e9, 3),
               verify_s=[round(t, 5) for t in t_verify], verify_median_s=round(med(t_verify), 5), verify_GBps=round(nbytes / med(t_verify) / 1e9, 1),
               create_handles_s=round(t_create, 4))
    tmp.cleanup()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
