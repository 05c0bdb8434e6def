"""Shared by tests/test_upconv_cpu.py and tests/test_hip_upconv.py: the literal form of the use_deconv=False upsampler
(nn.Upsample(scale (1,2,2), nearest) + nn.Conv3d (1,3,3)/s1/p(0,1,1) with a padding_mode, MT:169-172), evaluated per frame in the
dtype of its inputs, and the configurations of the goldens tools/gen_goldens_upconv.py writes."""
import torch
import torch.nn.functional as F_

MODES = ("zeros", "reflect", "replicate", "circular")
BORDER_MODE = {0: "zeros", 1: "reflect", 2: "circular"}       # a literal padding_mode for every dawn_conv_desc.border

TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=False, win_width=3)


def literal_upconv(img, w4, bias, mode):
    """img (F, Ci, H, W), w4 (Co, Ci, 3, 3), bias (Co,) or None -> (F, Co, 2H, 2W): interpolate -> pad(mode) -> conv2d."""
    u = F_.interpolate(img, scale_factor=2, mode="nearest")
    u = F_.pad(u, (1, 1, 1, 1), mode={"zeros": "constant"}.get(mode, mode))
    return F_.conv2d(u, w4, bias)


def literal_rows(x, Fr, H, W, w5, bias, mode):
    """The same on the kernels' layout, in fp64: x (Fr*H*W, Ci) rows, w5 (Co, Ci, 1, 3, 3) -> (Fr*2H*2W, Co) fp64."""
    img = x.double().reshape(Fr, H, W, -1).permute(0, 3, 1, 2)
    y = literal_upconv(img, w5[:, :, 0].double(), None if bias is None else bias.double(), mode)
    return y.permute(0, 2, 3, 1).reshape(Fr * 4 * H * W, -1)


def tiny_upconv_sd(tiny_sd, g):
    """State dict (denoise_fn.* keys) of a tiny use_deconv=False net: tiny_unet.npz's weights without the transposed conv, plus
    the two ups.0.4.1.* tensors of an upconv golden g."""
    sd = {k: v for k, v in tiny_sd.items() if not k.startswith("denoise_fn.ups.0.4.")}
    for k, v in g.items():
        if k.startswith("sd:"):
            sd[k[3:]] = torch.from_numpy(v)
    return sd
