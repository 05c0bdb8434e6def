"""`FlowDecoder`: the LFG latent-flow generator's inference entry points on the HIP kernels.

Mirrors `LFG/modules/generator.py::Generator` (GEN) for the two methods `FlowDiffusion.sample_one_video` calls --
`compute_fea` (GEN:132-136) and `forward_with_flow` (GEN:138-171) -- and adds `decode_clip`, the batched
equivalent of the reference's per-frame loop FD:372-385.  Built from the reference's own `generator` state_dict
(checkpoint['generator'], FD:122; key names unchanged), `skips=True` topology as in every shipped config.

What changes relative to the reference's execution (results are the same within fp32 rounding):
  * the source image is encoded ONCE per clip (the reference re-runs `first` + `down_blocks` for every frame,
    GEN:140-146), and the T frames are decoded as one batch per chunk instead of T batch-1 calls;
  * eval-mode BatchNorm + ReLU never take their own pass after an UpBlock2d convolution: they are applied by the
    kernel that consumes it (`warp_blend(prev_ab=...)`), which also performs the occlusion blend (GEN:80-87), the
    flow / occlusion resize (GEN:65-68, 81-82) and the next block's nearest x2 upsampling (UTIL:106);
  * every 3x3 convolution runs through `dawn_conv_gemm` (split-operand bf16 MFMA kernel, fp32-accurate);
  * the final 7x7 conv, sigmoid, last blend and the `deformed` output are one kernel writing (3,T,H,W) directly -- or, for the
    byte outputs (`decode_clip_u8`, `stream_frames_u8`), the same kernel writing (T,H,W,3) uint8 frames with no fp32 clip at all --
    or (`decode_clip_yuv420`, `stream_frames_yuv420`) writing what an encoder reads, (T, 3HW/2) planar YUV 4:2:0 (egress.py).

`use_ctx = True` hands the same launch sequence to the C-side decoder (include/dawn_hip.h: dawn_decoder_*, dawn_decode_clip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .egress import yuv420_frame_bytes, yuv420_from_rgb_u8
from .pack import pack_bf3, pack_kn

Tensor = torch.Tensor
BN_EPS = 1e-5        # SynchronizedBatchNorm2d / nn.BatchNorm2d default (UTIL:14)


def _bn_ab(sd, prefix: str, device):
    """Eval-mode BatchNorm as y = x*a + b (computed in fp64, stored fp32)."""
    g, be = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    m, v = sd[prefix + ".running_mean"].double(), sd[prefix + ".running_var"].double()
    a = g / torch.sqrt(v + BN_EPS)
    return a.float().to(device).contiguous(), (be - m * a).float().to(device).contiguous()


def _conv3_kn(w: Tensor) -> Tensor:
    """Conv2d weight (Co, Ci, 3, 3) -> (9*Ci, Co), k = (ky*3+kx)*Ci + ci (the order dawn_conv_gemm stages)."""
    Co, Ci, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw * Ci, Co)


@dataclass
class _Conv:
    w: Tensor
    ws: Optional[Tensor]
    bias: Tensor
    N: int
    a: Optional[Tensor] = None       # BatchNorm that FOLLOWS the conv (Same/Down/UpBlock2d)
    b: Optional[Tensor] = None


def _pack_conv3(sd, prefix: str, device, norm: Optional[str] = None) -> _Conv:
    w = sd[prefix + ".weight"].float()
    kn = _conv3_kn(w)
    c = _Conv(w=pack_kn(kn).to(device), ws=pack_bf3(kn).to(device) if kn.shape[0] % 16 == 0 else None,
              bias=sd[prefix + ".bias"].float().to(device).contiguous(), N=w.shape[0])
    if norm is not None:
        c.a, c.b = _bn_ab(sd, norm, device)
    return c


class FlowDecoder:
    """HIP-native `Generator.compute_fea` / `forward_with_flow` / clip decode.  `ops` is injectable for the CPU
    orchestration tests (oracle/ops_ref.RefOps); the default HipOps raises if libdawn_hip.so is missing."""

    def __init__(self, state_dict: Dict[str, Tensor], device, ops=None, chunk: int = 64):
        sd = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in state_dict.items()}
        if ops is None:
            from .ops import HipOps
            ops = HipOps()
        self.ops = ops
        self.device = torch.device(device)
        self.chunk = chunk
        dev = self.device
        w1 = sd["first.conv.weight"].float()                                       # (C0, 3, 7, 7)
        self.C0 = w1.shape[0]
        self.first_w3 = w1.permute(2, 3, 1, 0).reshape(147, self.C0).contiguous().to(dev)
        self.first_bias = sd["first.conv.bias"].float().to(dev)
        self.first_ab = _bn_ab(sd, "first.norm", dev)
        self.downs: List[_Conv] = []
        while f"down_blocks.{len(self.downs)}.conv.weight" in sd:
            i = len(self.downs)
            self.downs.append(_pack_conv3(sd, f"down_blocks.{i}.conv", dev, f"down_blocks.{i}.norm"))
        self.ups: List[_Conv] = []
        while f"up_blocks.{len(self.ups)}.conv.weight" in sd:
            i = len(self.ups)
            self.ups.append(_pack_conv3(sd, f"up_blocks.{i}.conv", dev, f"up_blocks.{i}.norm"))
        if len(self.ups) != len(self.downs):
            raise ValueError("LFG generator: up/down block counts differ")
        self.bott = []
        while f"bottleneck.r{len(self.bott)}.conv1.weight" in sd:
            p = f"bottleneck.r{len(self.bott)}"
            self.bott.append((_bn_ab(sd, p + ".norm1", dev), _pack_conv3(sd, p + ".conv1", dev),
                              _bn_ab(sd, p + ".norm2", dev), _pack_conv3(sd, p + ".conv2", dev)))
        wf = sd["final.weight"].float()                                            # (3, C0, 7, 7)
        if wf.shape[0] != 3 or wf.shape[1] % 8 != 0:
            raise ValueError("LFG generator: final conv must be (3, C % 8 == 0, 7, 7)")
        Cf = wf.shape[1]
        # [tap][C/4][3 outputs][4 channels]
        self.final_w7 = wf.permute(2, 3, 1, 0).reshape(49, Cf // 4, 4, 3).permute(0, 1, 3, 2).contiguous().to(dev)
        self.final_bias = sd["final.bias"].float().to(dev).contiguous()
        self._bias_maps: Dict[int, Tensor] = {}

    @classmethod
    def from_generator(cls, generator, device=None, **kw) -> "FlowDecoder":
        """Build from the reference's (unchanged) `Generator` module: only its state_dict is read."""
        sd = generator.state_dict()
        if device is None:
            device = next(iter(sd.values())).device
        return cls(sd, device, **kw)

    # ------------------------------------------------------------------ encoder (once per clip)
    def _conv3(self, x: Tensor, c: _Conv, F: int, H: int, W: int, res: Optional[Tensor] = None) -> Tensor:
        return self.ops.conv_gemm(x, c.w, c.N, F=F, Hi=H, Wi=W, KH=3, KW=3, stride=1, pad=1, bias=c.bias, res=res,
                                  w_bf3=c.ws)

    def encode(self, img: Tensor) -> List[Tensor]:
        """img (3,H,W) -> channels-last skips [(H*W, C0), (H/2*W/2, C1), ...]   (GEN:140-146)."""
        _, H, W = img.shape
        if H % (1 << len(self.downs)) or W % (1 << len(self.downs)):
            raise ValueError(f"image size {H}x{W} is not divisible by 2^{len(self.downs)}")
        n = H * W
        if n not in self._bias_maps:
            self._bias_maps[n] = self.first_bias.view(1, -1).expand(n, -1).contiguous()
        x3 = img.float().contiguous().view(3, 1, H, W)
        y = self.ops.init_conv_x(x3, self.first_w3, self._bias_maps[n], 1, H, W, self.C0)
        cur = self.ops.affine_act(y, self.first_ab[0], self.first_ab[1], 1)
        skips = [cur]
        for d in self.downs:
            z = self._conv3(cur, d, 1, H, W)
            cur = self.ops.bn_relu_pool2(z, d.a, d.b, 1, H, W)
            H, W = H // 2, W // 2
            skips.append(cur)
        return skips

    def compute_fea(self, source_image: Tensor) -> Tensor:
        """GEN:132-136: (B,3,H,W) -> (B,Cb,H/2^n,W/2^n)."""
        B, _, H, W = source_image.shape
        k = 1 << len(self.downs)
        outs = []
        for b in range(B):
            if self._via_ctx(source_image):
                outs.append(self._evaluator().encode(source_image[b].float().contiguous(), want_fea=True)[1])
                continue
            f = self.encode(source_image[b])[-1]
            outs.append(f.view(H // k, W // k, -1).permute(2, 0, 1))
        return torch.stack(outs, 0).contiguous()

    # ------------------------------------------------------------------ decoder
    def _decode_frames(self, skips: List[Tensor], src: Tensor, H: int, W: int, g: Tensor, cf: Tensor, out_vid: Optional[Tensor],
                       warped_vid: Optional[Tensor], frames: Optional[Tensor] = None, mean=(0.0, 0.0, 0.0),
                       bgr: bool = False, yuv: Optional[Tensor] = None) -> None:
        """g (2,n,h,w) view, cf (n,h,w); writes out_vid / warped_vid (3,n,H,W) views and / or frames (n,H,W,3) uint8.  GEN:152-167.
        With `frames` alone the last launch is the fused final_conv_blend_u8 where the op set has it (no fp32 frame is written);
        otherwise final_conv_blend followed by frames_to_u8 on the chunk -- which is also the definition of the fused op's result.
        `yuv` (n, 3HW/2) uint8, alone: the fused final_conv_blend_yuv420 where the op set has it; otherwise final_conv_blend ->
        frames_to_u8 (RGB) -> egress.yuv420_from_rgb_u8, the definition of that op's result."""
        ops = self.ops
        n = g.shape[1]
        k = 1 << len(self.downs)
        Hc, Wc = H // k, W // k
        x = ops.warp_blend(skips[-1], Hc, Wc, g, cf)                                # GEN:154 (no previous input)
        for (ab1, c1, ab2, c2) in self.bott:                                        # GEN:156, UTIL:83-91
            y = ops.affine_act(x, ab1[0], ab1[1], 1)
            z = self._conv3(y, c1, n, Hc, Wc)
            y = ops.affine_act(z, ab2[0], ab2[1], 1)
            x = self._conv3(y, c2, n, Hc, Wc, res=x)
        prev, prev_ab = x, None
        for i, up in enumerate(self.ups):                                           # GEN:157-160
            u = ops.warp_blend(skips[-(i + 1)], Hc, Wc, g, cf, prev=prev, prev_ab=prev_ab, up2=True)
            Hc, Wc = 2 * Hc, 2 * Wc
            prev = self._conv3(u, up, n, Hc, Wc)                                    # UTIL:107; its BN+ReLU ride on the consumer
            prev_ab = (up.a, up.b)
        xf = ops.warp_blend(skips[0], H, W, g, cf, prev=prev, prev_ab=prev_ab)      # GEN:161-162
        if yuv is not None and hasattr(ops, "final_conv_blend_yuv420"):
            ops.final_conv_blend_yuv420(xf, H, W, self.final_w7, self.final_bias, src, g, cf, yuv, mean=mean)
            return
        if yuv is None and frames is not None and out_vid is None and hasattr(ops, "final_conv_blend_u8"):
            ops.final_conv_blend_u8(xf, H, W, self.final_w7, self.final_bias, src, g, cf, frames, mean=mean, bgr=bgr)
            return
        if out_vid is None:
            out_vid = torch.empty(3, n, H, W, device=xf.device, dtype=torch.float32)
            warped_vid = torch.empty_like(out_vid)
        ops.final_conv_blend(xf, H, W, self.final_w7, self.final_bias, src, g, cf, out_vid, warped_vid)   # GEN:163-167, 152
        if frames is not None:
            frames.copy_(ops.frames_to_u8(out_vid, mean=mean, bgr=bgr))
        if yuv is not None:
            yuv.copy_(yuv420_from_rgb_u8(ops.frames_to_u8(out_vid, mean=mean, bgr=False)))

    # ---- the two hosts of the launch sequence: this file's orchestration, or the C-side decoder (use_ctx; ctx.DecoderEvaluator)
    use_ctx = False      # True: GPU clips go through dawn_decoder_encode / dawn_decode_clip (bit-identical to the orchestration here)

    def _evaluator(self):
        if getattr(self, "_ctx_eval", None) is None:
            from .ctx import DecoderEvaluator
            self._ctx_eval = DecoderEvaluator(self)
        return self._ctx_eval

    def _via_ctx(self, t: Tensor) -> bool:
        return bool(self.use_ctx) and t.is_cuda

    def _begin_clip(self, src: Tensor):
        """Once per clip: the encoder skips, as a list (orchestration here) or as the C-side decoder's skip memory."""
        if self._via_ctx(src):
            return self._evaluator().encode(src)[0]
        return self.encode(src)

    def _chunk(self, state, src: Tensor, H: int, W: int, g: Tensor, cf: Tensor, out_vid: Optional[Tensor],
               warped_vid: Optional[Tensor], frames: Optional[Tensor] = None, mean=(0.0, 0.0, 0.0), bgr: bool = False,
               chunk: Optional[int] = None, yuv: Optional[Tensor] = None) -> None:
        """Frames of g / cf (any number: the C side splits them into chunks itself) into the given outputs."""
        if isinstance(state, list):
            return self._decode_frames(state, src, H, W, g, cf, out_vid, warped_vid, frames, mean, bgr, yuv)
        _, n, h, w = g.shape
        self._evaluator().decode(src, state, T=n, h=h, w=w, chunk=chunk or n, grid=g, conf=cf, out_vid=out_vid,
                                 warped_vid=warped_vid, frames=frames, mean=mean, bgr=bgr, yuv=yuv)

    @torch.no_grad()
    def decode_clip(self, sample_img: Tensor, grid: Tensor, conf: Tensor, chunk: Optional[int] = None) -> Dict[str, Tensor]:
        """The loop FD:372-385 for whole clips: sample_img (B,3,H,W), grid (B,2,T,h,w) = `sample_vid_grid`,
        conf (B,1,T,h,w) = `sample_vid_conf` -> {sample_out_vid, sample_warped_vid} (B,3,T,H,W)."""
        B, _, T, h, w = grid.shape
        _, _, H, W = sample_img.shape
        chunk = chunk or self.chunk
        grid = grid.float().contiguous()
        conf = conf.float().contiguous()
        out_vid = torch.empty(B, 3, T, H, W, device=grid.device, dtype=torch.float32)
        warped = torch.empty_like(out_vid)
        for b in range(B):
            src = sample_img[b].float().contiguous()
            state = self._begin_clip(src)
            if not isinstance(state, list):                                         # C side: one call, it runs the chunk loop
                self._chunk(state, src, H, W, grid[b], conf[b, 0], out_vid[b], warped[b], chunk=chunk)
                continue
            for t0 in range(0, T, chunk):
                t1 = min(T, t0 + chunk)
                self._decode_frames(state, src, H, W, grid[b, :, t0:t1], conf[b, 0, t0:t1], out_vid[b, :, t0:t1],
                                    warped[b, :, t0:t1])
        return {"sample_out_vid": out_vid, "sample_warped_vid": warped}

    @torch.no_grad()
    def decode_clip_u8(self, sample_img: Tensor, grid: Tensor, conf: Tensor, *, mean=(0.0, 0.0, 0.0), bgr: bool = False,
                       chunk: Optional[int] = None) -> Tensor:
        """decode_clip + the frame egress without the fp32 clips: -> (B,T,H,W,3) uint8 on the inputs' device, byte
        for byte `ops.frames_to_u8(decode_clip(...)["sample_out_vid"][b], mean, bgr)`.  `mean` = the config's 0..255 offsets."""
        B, _, T, h, w = grid.shape
        _, _, H, W = sample_img.shape
        chunk = chunk or self.chunk
        grid = grid.float().contiguous()
        conf = conf.float().contiguous()
        out = torch.empty(B, T, H, W, 3, device=grid.device, dtype=torch.uint8)
        for b in range(B):
            src = sample_img[b].float().contiguous()
            state = self._begin_clip(src)
            if not isinstance(state, list):
                self._chunk(state, src, H, W, grid[b], conf[b, 0], None, None, out[b], mean, bgr, chunk=chunk)
                continue
            for t0 in range(0, T, chunk):
                t1 = min(T, t0 + chunk)
                self._decode_frames(state, src, H, W, grid[b, :, t0:t1], conf[b, 0, t0:t1], None, None, out[b, t0:t1], mean, bgr)
        return out

    @torch.no_grad()
    def decode_clip_yuv420(self, sample_img: Tensor, grid: Tensor, conf: Tensor, *, mean=(0.0, 0.0, 0.0),
                           chunk: Optional[int] = None) -> Tensor:
        """decode_clip_u8 for an encoder: -> (B,T,3HW/2) uint8 on the inputs' device, every frame planar YUV 4:2:0 (I420: Y, then U, then
        V; BT.601 limited range, 2x2 box chroma -- the definition in egress.py), byte for byte
        `egress.yuv420_from_rgb_u8(decode_clip_u8(..., mean=mean, bgr=False)[b])`.  Neither fp32 clips nor RGB bytes are written where
        the op set has the fused kernel.  Even H, W % 4 == 0."""
        B, _, T, h, w = grid.shape
        _, _, H, W = sample_img.shape
        chunk = chunk or self.chunk
        grid = grid.float().contiguous()
        conf = conf.float().contiguous()
        out = torch.empty(B, T, yuv420_frame_bytes(H, W), device=grid.device, dtype=torch.uint8)
        for b in range(B):
            src = sample_img[b].float().contiguous()
            state = self._begin_clip(src)
            if not isinstance(state, list):
                self._chunk(state, src, H, W, grid[b], conf[b, 0], None, None, None, mean, chunk=chunk, yuv=out[b])
                continue
            for t0 in range(0, T, chunk):
                t1 = min(T, t0 + chunk)
                self._decode_frames(state, src, H, W, grid[b, :, t0:t1], conf[b, 0, t0:t1], None, None, None, mean, yuv=out[b, t0:t1])
        return out

    def _stream_chunks(self, sample_img: Tensor, grid: Tensor, conf: Tensor, chunk: Optional[int], item: int, frame_shape, decode):
        """The chunk loop both byte streams share: yields (t0, host ndarray (n, *frame_shape) uint8).  decode(state, src, H, W, g, cf,
        buf) writes the frames of one chunk into buf (n, *frame_shape).  On the GPU the device->host copy of a chunk runs on a side
        stream into pinned memory while the next chunk decodes; the consumer waits for that chunk's copy event only (no device-wide
        synchronise), and no clip-sized tensor exists on the device: two chunk-sized byte buffers plus the chunk's activations."""
        _, _, T, h, w = grid.shape
        _, _, H, W = sample_img.shape
        chunk = max(1, min(chunk or self.chunk, T))
        g = grid[item].float().contiguous()
        cf = conf[item, 0].float().contiguous()
        src = sample_img[item].float().contiguous()
        state = self._begin_clip(src)
        spans = [(t0, min(T, t0 + chunk)) for t0 in range(0, T, chunk)]
        if not g.is_cuda:
            for t0, t1 in spans:
                fr = torch.empty(t1 - t0, *frame_shape, dtype=torch.uint8)
                decode(state, src, H, W, g[:, t0:t1], cf[t0:t1], fr)
                yield t0, fr.numpy()
            return
        main = torch.cuda.current_stream(g.device)
        side = torch.cuda.Stream(device=g.device)
        dev = [torch.empty(chunk, *frame_shape, device=g.device, dtype=torch.uint8) for _ in range(2)]
        host = [torch.empty(chunk, *frame_shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        copied = [None, None]                          # event of the last copy out of dev[k] / into host[k]
        pending = None
        try:
            for i, (t0, t1) in enumerate(spans):
                k, n = i & 1, t1 - t0
                if copied[k] is not None:
                    main.wait_event(copied[k])         # dev[k] is free once chunk i - 2 has left it
                decode(state, src, H, W, g[:, t0:t1], cf[t0:t1], dev[k][:n])
                decoded = torch.cuda.Event()
                decoded.record(main)
                with torch.cuda.stream(side):
                    side.wait_event(decoded)
                    host[k][:n].copy_(dev[k][:n], non_blocking=True)
                    copied[k] = torch.cuda.Event()
                    copied[k].record(side)
                if pending is not None:                # hand out chunk i - 1 while chunk i decodes
                    pt0, pn, pk = pending
                    copied[pk].synchronize()
                    yield pt0, host[pk][:pn].numpy()
                pending = (t0, n, k)
            if pending is not None:
                pt0, pn, pk = pending
                copied[pk].synchronize()
                yield pt0, host[pk][:pn].numpy()
        finally:
            side.synchronize()                         # an abandoned generator must not free buffers under a copy in flight

    @torch.no_grad()
    def stream_frames_u8(self, sample_img: Tensor, grid: Tensor, conf: Tensor, *, mean=(0.0, 0.0, 0.0), bgr: bool = False,
                         chunk: Optional[int] = None, item: int = 0):
        """Generator over the chunks of batch item `item`: yields (t0, frames) with frames a host ndarray (n,H,W,3) uint8, the bytes
        of decode_clip_u8 for the frames [t0, t0 + n), in order.  On the GPU the device->host copy of a chunk runs on a side stream
        into pinned memory while the next chunk decodes; the consumer waits for that chunk's copy event only (no device-wide
        synchronise), and no clip-sized tensor exists on the device: two chunk-sized byte buffers plus the chunk's activations.
        A YIELDED ARRAY IS VALID UNTIL THE NEXT `next()` ONLY: it aliases one of two pinned staging buffers, which the chunk after
        the next one overwrites -- copy it if it has to live longer.  CPU tensors: the plain loop, every chunk its own array."""
        _, _, H, W = sample_img.shape

        def decode(state, src, H, W, g, cf, buf):
            self._chunk(state, src, H, W, g, cf, None, None, buf, mean, bgr)
        yield from self._stream_chunks(sample_img, grid, conf, chunk, item, (H, W, 3), decode)

    @torch.no_grad()
    def stream_frames_yuv420(self, sample_img: Tensor, grid: Tensor, conf: Tensor, *, mean=(0.0, 0.0, 0.0),
                             chunk: Optional[int] = None, item: int = 0):
        """stream_frames_u8 for an encoder: yields (t0, frames) with frames a host ndarray (n, 3HW/2) uint8, the bytes of
        decode_clip_yuv420 for the frames [t0, t0 + n), in order -- `frames.tobytes()` is what `-f rawvideo -pix_fmt yuv420p` reads.
        Half the device->host bytes of the RGB stream; the same staging, and the same rule: A YIELDED ARRAY IS VALID UNTIL THE NEXT
        `next()` ONLY."""
        _, _, H, W = sample_img.shape

        def decode(state, src, H, W, g, cf, buf):
            self._chunk(state, src, H, W, g, cf, None, None, None, mean, yuv=buf)
        yield from self._stream_chunks(sample_img, grid, conf, chunk, item, (yuv420_frame_bytes(H, W),), decode)

    @torch.no_grad()
    def forward_with_flow(self, source_image: Tensor, optical_flow: Tensor, occlusion_map: Tensor) -> Dict[str, Tensor]:
        """GEN:138-171 with the reference's signature: source_image (B,3,H,W), optical_flow (B,h,w,2),
        occlusion_map (B,1,h,w); every batch item has its own source image."""
        grid = optical_flow.permute(0, 3, 1, 2).unsqueeze(2)                        # (B,2,1,h,w)
        conf = occlusion_map.unsqueeze(2)                                           # (B,1,1,h,w)
        o = self.decode_clip(source_image, grid, conf)
        return {"prediction": o["sample_out_vid"][:, :, 0], "deformed": o["sample_warped_vid"][:, :, 0]}
