#!/usr/bin/env python3
"""Goldens of the `use_deconv=False` UNet (nn.Upsample(scale (1,2,2), nearest) + nn.Conv3d (1,3,3), MT:169-172), produced by
RUNNING THE REFERENCE module in the build container.

    DAWN_REFERENCE=<reference checkout> python tools/gen_goldens_upconv.py [case ...]        # cases: reflect zeros full (default: all)

    reflect / zeros : the `TINY` configuration with use_deconv=False and that padding_mode.  Weights = tiny_unet.npz without its
                      ups.0.4.* (the transposed conv) plus a seeded ups.0.4.1.weight / .bias -- the fixture stores those two
                      tensors only; inputs = those of tiny_unet.npz (not stored again); output = forward_with_cond_scale(...,
                      cond_scale=1.0).  tiny_unet_upconv_<mode>.npz
    full            : the shipped architecture (dim_mults (1,2,4,8), window 40), padding_mode="reflect", T = 50, h = w = 32: the
                      smallest clip at which one forward runs both kernel families (the 16x16 -> 32x32 up conv has 50 * 256 = 12,800
                      rows and takes the split row-accumulator kernel, the 8x8 and 4x4 levels the fp32 kernels).  Weights = the
                      deterministic `init_seed=0` weights of this repository's Unet3D(use_deconv=False), loaded into the reference
                      module; inputs = tests/fullsize_cases.build_inputs(50, 32) (seeded: rebuilt bit-identically by the test, the
                      fixture holds their checksum); output = forward_with_cond_scale(..., cond_scale=1.0).  upconv_full_T50.npz

Data only; the reference's Python never leaves this container.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAWN_REFERENCE")
if not REF:
    sys.exit("set DAWN_REFERENCE to the checkout of the reference project")
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_stubs"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import DM_3.modules.video_flow_diffusion_multiGPU_v0_crema_plus_faceemb_ca_multi_test as MT  # noqa: E402

torch.set_grad_enabled(False)

TINY = dict(dim=16, cond_dim=24 + 6 + 2, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12,
            channels=3 + 16, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2),
            use_hubert_audio_cond=True, learn_null_cond=False, use_final_activation=False,
            use_deconv=False, win_width=3)
FULL_T, FULL_H, FULL_TIME = 50, 32, 627
UP_KEYS = ("ups.0.4.1.weight", "ups.0.4.1.bias")


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.3f} MB")


def gen_tiny(mode):
    g = np.load(os.path.join(OUT, "tiny_unet.npz"))
    sd = {k[len("sd:denoise_fn."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd:denoise_fn.")}
    u = MT.DynamicNfUnet3D(default_num_frames=12, **TINY, padding_mode=mode)
    new = [k for k in u.state_dict() if k not in sd]
    gone = [k for k in sd if k not in u.state_dict()]
    assert sorted(new) == sorted(UP_KEYS) and sorted(gone) == ["ups.0.4.bias", "ups.0.4.weight"], (new, gone)
    gen = torch.Generator().manual_seed(4242)                  # (the same two tensors for both modes)
    for k in UP_KEYS:
        shape = u.state_dict()[k].shape
        sd[k] = torch.randn(shape, generator=gen) * (0.08 if k.endswith("weight") else 0.05)
    for k in gone:
        del sd[k]
    u.load_state_dict(sd, strict=True)
    u.update_num_frames(12)
    u.eval()
    x, t, cond = (torch.from_numpy(g[k]) for k in ("x", "time", "cond"))
    y = u.forward_with_cond_scale(x, t, cond=cond, cond_scale=1.0)
    ups_shapes = {k: tuple(v.shape) for k, v in u.state_dict().items() if k.startswith("ups.")}
    print(f"tiny {mode}: max|y| = {float(y.abs().max()):.4f}, max|y - y(deconv golden)| = {float((y - torch.from_numpy(g['y'])).abs().max()):.4f}")
    save(f"tiny_unet_upconv_{mode}.npz", y=y.numpy(), padding_mode=np.array(mode),
         ups_keys=np.array(sorted(ups_shapes)), ups_shapes=np.array([",".join(map(str, ups_shapes[k])) for k in sorted(ups_shapes)]),
         **{"sd:denoise_fn." + k: sd[k].numpy() for k in UP_KEYS})


def gen_full():
    import dawn_pytorch_amd as D
    from fullsize_cases import KW, build_inputs, checksum
    kw = {**KW, "use_deconv": False, "padding_mode": "reflect"}
    T, h = FULL_T, FULL_H
    ours = D.DynamicNfUnet3D(default_num_frames=8, **kw, init_seed=0)
    sd = ours.state_dict()
    fea272, cond, x3 = build_inputs(T, h)
    u = MT.DynamicNfUnet3D(default_num_frames=T, **kw)
    u.update_num_frames(T)
    u.load_state_dict(sd, strict=True)
    u.eval()
    x = torch.cat((x3, fea272[:, :, None].expand(-1, -1, T, -1, -1)), dim=1).contiguous()
    t0 = time.time()
    y = u.forward_with_cond_scale(x, torch.tensor([FULL_TIME]), cond=cond, cond_scale=1.0)
    dt = time.time() - t0
    print(f"full: reference forward T={T} h={h}: {dt:.1f} s, max|y| = {float(y.abs().max()):.4f}")
    save("upconv_full_T50.npz", T=T, h=h, time=np.array([FULL_TIME]), padding_mode=np.array("reflect"), inputs_seed=123,
         y=y[0].numpy(), weights_checksum=checksum(sd.values()), inputs_checksum=checksum([fea272, cond, x3]), ref_seconds=dt)


if __name__ == "__main__":
    cases = {"reflect": lambda: gen_tiny("reflect"), "zeros": lambda: gen_tiny("zeros"), "full": gen_full}
    for name in sys.argv[1:] or list(cases):
        cases[name]()
