#!/usr/bin/env python3
"""Stage-wise golden vectors for the LFG motion encode, made by IMPORTING THE REFERENCE's RegionPredictor,
BGMotionPredictor and Generator (LFG/modules/) in the build container and running them as FlowDiffusion.forward does (FD:248-262).

    python tools/gen_goldens_motion.py      # writes tests/golden/motion_tiny_sd.npz, motion_A.npz, motion_B.npz (data only)
    python tools/gen_goldens_motion.py N    # writes tests/golden/motion_N.npz alone (any names of motion_cases.CASES / E2E_CASES), from
                                            # the same seeded models; no other file is touched

The cases of motion_cases.E2E_CASES (N: 96 x 128, not square) hold the reference's optical_flow and occlusion_map only.

Inputs are not stored: tests/motion_cases.frames_u8 makes them (bytes from an integer formula).  Weights: narrow instances of the shipped
architecture (motion_cases.TINY / GEN_TINY), every parameter and BatchNorm statistic randomised -- the constructors zero `fc` -- and
rounded to fp16 values, stored as fp16 (exact in fp32).  The `regions` conv is rescaled so that its output has a standard deviation of
0.3 on case A's source (heatmaps of a few dozen pixels: covariances that are neither degenerate nor isotropic).

Stage-wise: a stage's golden holds the reference's own inputs of that stage (its upstream values, captured by hooks) beside its outputs, so
each kernel is tested from them.  To keep the files small the largest arrays are kept for a subset of frames only (`*_frames` says which):
the hourglass input and the decoded prediction for the last frame, and in case B (256 x 256) only the stages that depend on the 4096-pixel
map (the driving frames' `regions` output and moments, the downsampled source, the end-to-end flow and occlusion).  The tool prints, per case, the share of regions a test may skip (relative eigen-gap < motion_cases.GAP_MIN in either frame, or
det(u) > 0 in the reference's SVD); it fails above motion_cases.SKIP_CAP -- pick another seed then."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAWN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_stubs"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from LFG.modules.bg_motion_predictor import BGMotionPredictor  # noqa: E402
from LFG.modules.generator import Generator  # noqa: E402
from LFG.modules.region_predictor import RegionPredictor  # noqa: E402

import motion_cases as mc  # noqa: E402

torch.set_grad_enabled(False)
SEED = 5


def randomise(mod, g):
    for name, buf in mod.named_buffers():
        if name.endswith("running_mean"):
            buf.copy_(torch.randn(buf.shape, generator=g) * 0.2)
        elif name.endswith("running_var"):
            buf.copy_(torch.rand(buf.shape, generator=g) * 1.5 + 0.25)
    for _, p in mod.named_parameters():
        p.add_(torch.randn(p.shape, generator=g) * 0.05)
        p.copy_(p.half().float())
    for name, buf in mod.named_buffers():
        if name.endswith(("running_mean", "running_var")):
            buf.copy_(buf.half().float())
    mod.eval()


def build():
    torch.manual_seed(SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    rp = RegionPredictor(num_regions=mc.R, num_channels=3, temperature=mc.TEMPERATURE, estimate_affine=True, scale_factor=1 / mc.S,
                         pca_based=True, **mc.TINY)
    bg = BGMotionPredictor(num_channels=3, bg_type="affine", **mc.TINY)
    gen = Generator(num_channels=3, num_regions=mc.R, skips=True, revert_axis_swap=True,
                    pixelwise_flow_predictor_params=dict(scale_factor=1 / mc.S, use_deformed_source=True, use_covar_heatmap=True,
                                                         estimate_occlusion_map=True, **mc.TINY), **mc.GEN_TINY)
    for m in (rp, bg, gen):
        randomise(m, g)
    # regions: output standard deviation 0.3 on case A's source
    src = mc.to_float(mc.frames_u8("A")[0]).unsqueeze(0)
    rp.regions.bias.zero_()
    std = rp.regions(rp.predictor(rp.down(src))).std()
    rp.regions.weight.mul_(0.3 / std)
    rp.regions.weight.copy_(rp.regions.weight.half().float())
    return rp, bg, gen


def run_case(name, rp, bg, gen):
    c = mc.CASES[name] if name in mc.CASES else mc.E2E_CASES[name]
    T = c["T"]
    src_u8, drv_u8 = mc.frames_u8(name)
    src, drv = mc.to_float(src_u8).unsqueeze(0), mc.to_float(drv_u8)
    cap = {}
    hooks = [rp.down.register_forward_hook(lambda m, i, o: cap.setdefault("down", []).append(o)),
             rp.regions.register_forward_hook(lambda m, i, o: cap.setdefault("regions", []).append(o)),
             bg.encoder.register_forward_hook(lambda m, i, o: cap.__setitem__("bg_last", o[-1])),
             gen.pixelwise_flow_predictor.hourglass.register_forward_pre_hook(lambda m, i: cap.__setitem__("pf_in", i[0])),
             gen.pixelwise_flow_predictor.mask.register_forward_hook(lambda m, i, o: cap.__setitem__("mask", o)),
             gen.pixelwise_flow_predictor.occlusion.register_forward_hook(lambda m, i, o: cap.__setitem__("occ", o))]
    ref_tmp = src.repeat(T, 1, 1, 1)                                                    # FD:252
    sp = rp(ref_tmp)
    dp = rp(drv)
    bgp = bg(ref_tmp, drv)
    out = gen(ref_tmp, source_region_params=sp, driving_region_params=dp, bg_params=bgp)
    for hk in hooks:
        hk.remove()
    h, w = cap["down"][0].shape[2:]
    # the share of regions a test may skip
    gap = torch.minimum(mc.eigen_gap(sp["covar"][0]).unsqueeze(0).expand(T, -1), mc.eigen_gap(dp["covar"]))
    det = torch.det(torch.cat((sp["u"][:mc.R], dp["u"]), 0))
    skip = (gap < mc.GAP_MIN) | (det[mc.R:].view(T, mc.R) > 0) | (det[:mc.R] > 0).unsqueeze(0)
    share = float(skip.float().mean())
    print(f"case {name}: {h} x {w} map, skippable regions {int(skip.sum())} of {skip.numel()} ({share:.1%}); min relative eigen-gap "
          f"{float(gap.min()):.3g}; det(u) > 0: {int((det > 0).sum())} of {det.numel()}; covar diag range "
          f"[{float(dp['covar'].diagonal(dim1=-2, dim2=-1).min()):.3g}, {float(dp['covar'].diagonal(dim1=-2, dim2=-1).max()):.3g}]; "
          f"occlusion [{float(out['occlusion_map'].min()):.3f}, {float(out['occlusion_map'].max()):.3f}]")
    assert share <= mc.SKIP_CAP, "too many ill-conditioned regions: pick another seed"
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    last = [T - 1]
    a = dict(
        # region predictor: source (frame axis 1) and driving
        drv_regions=cap["regions"][1],
        src_shift=sp["shift"][0], src_covar=sp["covar"][0], src_affine=sp["affine"][0], src_u=sp["u"][:mc.R],
        drv_shift=dp["shift"], drv_covar=dp["covar"], drv_affine=dp["affine"], drv_u=dp["u"].view(T, mc.R, 2, 2),
        down_src=cap["down"][0][0],
        optical_flow=out["optical_flow"], occlusion_map=out["occlusion_map"], bg_params=bgp)
    if name in mc.E2E_CASES:
        assert tuple(out["optical_flow"].shape) == (T, h, w, 2) and h != w
        a = dict(optical_flow=out["optical_flow"], occlusion_map=out["occlusion_map"])
    if name == "A":
        a.update(src_regions=cap["regions"][0][:1], down_drv=cap["down"][1], bg_last=cap["bg_last"], pf_in=cap["pf_in"][last], pf_in_frames=np.array(last),
                 mask_occ=torch.cat((cap["mask"], cap["occ"]), 1), prediction=out["prediction"][last], deformed=out["deformed"][last],
                 prediction_frames=np.array(last))
    arrs = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in a.items()}
    path = os.path.join(ROOT, "tests", "golden", f"motion_{name}.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays")


def main():
    rp, bg, gen = build()
    if len(sys.argv) > 1:                                               # the named cases alone
        for name in sys.argv[1:]:
            run_case(name, rp, bg, gen)
        return
    arrs = {}
    for tag, m in (("generator", gen), ("region_predictor", rp), ("bg_predictor", bg)):
        for k, v in m.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            keep32 = k.endswith("down.weight")                      # the antialias buffers are no fp16 values
            assert keep32 or torch.equal(v.half().float(), v), k
            arrs[f"{tag}/{k}"] = v.numpy() if keep32 else v.half().numpy()
    path = os.path.join(ROOT, "tests", "golden", "motion_tiny_sd.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays")
    for name in mc.CASES:
        run_case(name, rp, bg, gen)


if __name__ == "__main__":
    main()
