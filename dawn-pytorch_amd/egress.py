"""Frame egress formats past the RGB bytes: what an encoder reads.

`yuv420_from_rgb_u8` states the yuv420p definition of include/dawn_hip.h (dawn_frames_to_yuv420) in torch integer ops, on any
device.  It is what an op set without the HIP kernels runs (oracle/ops_ref.RefOps: the CPU orchestration composes final_conv_blend ->
frames_to_u8 -> this); `HipOps` has `final_conv_blend_yuv420` / `frames_to_yuv420` and never comes here.

    Y  = (( 66*R + 129*G +  25*B + 128) >> 8) + 16                      per pixel
    R' = (R00 + R01 + R10 + R11 + 2) >> 2   (same for G', B')           per 2x2 block (centre-sited box average)
    U  = ((-38*R' -  74*G' + 112*B' + 128) >> 8) + 128
    V  = ((112*R' -  94*G' -  18*B' + 128) >> 8) + 128

BT.601 limited range, `>>` an arithmetic shift.  I420: every frame is Y (H*W bytes), U ((H/2)*(W/2)), V (the same), contiguous;
frames back to back."""
from __future__ import annotations

import torch

Tensor = torch.Tensor


def yuv420_frame_bytes(H: int, W: int) -> int:
    if H <= 0 or W <= 0 or H % 2 or W % 4:
        raise ValueError(f"yuv420p needs an even H and W % 4 == 0, not {H}x{W}")
    return H * W * 3 // 2


def yuv420_from_rgb_u8(frames: Tensor) -> Tensor:
    """frames (T,H,W,3) uint8, RGB order -> (T, 3*H*W/2) uint8, I420."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("yuv420_from_rgb_u8: frames must be (T,H,W,3) uint8")
    T, H, W, _ = frames.shape
    out = torch.empty(T, yuv420_frame_bytes(H, W), dtype=torch.uint8, device=frames.device)
    c = frames.to(torch.int32)
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    out[:, :H * W] = (((66 * R + 129 * G + 25 * B + 128) >> 8) + 16).reshape(T, H * W).to(torch.uint8)
    q = (c.view(T, H // 2, 2, W // 2, 2, 3).sum(dim=(2, 4)) + 2) >> 2                      # (T,H/2,W/2,3)
    R, G, B = q[..., 0], q[..., 1], q[..., 2]
    n = (H // 2) * (W // 2)
    out[:, H * W:H * W + n] = (((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128).reshape(T, n).to(torch.uint8)
    out[:, H * W + n:] = (((112 * R - 94 * G - 18 * B + 128) >> 8) + 128).reshape(T, n).to(torch.uint8)
    return out
