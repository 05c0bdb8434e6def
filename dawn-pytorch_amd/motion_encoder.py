"""`MotionEncoder`: the encode half of the frozen LFG on the HIP kernels -- a source image and the frames of a driving
video to the flow and occlusion latent that the diffusion model samples and `FlowDecoder` decodes.

Mirrors what `FlowDiffusion.forward` runs under no_grad on `real_vid` (FD:248-262): `RegionPredictor` (RP = LFG/modules/region_predictor.py)
on the source and on every frame, `BGMotionPredictor` (BG = bg_motion_predictor.py) on every (source, frame) pair, and
`Generator.forward`'s `PixelwiseFlowPredictor` (PF = pixelwise_flow_predictor.py).  Built from the LFG checkpoint's three state_dicts
(`generator`, `region_predictor`, `bg_predictor`; key names unchanged) for the shipped configuration -- pca_based regions with affine
estimation, revert_axis_swap, an 'affine' background, deformed source, covariance heatmaps, an occlusion map -- and nothing else: any other
configuration is refused with a message.

What changes relative to the reference's execution (results are the same within fp32 rounding):
  * the source side -- its region parameters, its downsampled image, its half of the background encoder's first convolution -- is
    computed ONCE per clip (the reference repeats the source T times through both predictors, FD:252-256);
  * the T frames are a batch, processed in chunks, so the workspace does not grow with T;
  * the 2x2 SVD is a closed form on the device (the reference moves every covariance to the CPU for torch.svd, RP:21);
  * the heatmap tensor, the R + 1 sparse-motion grids and the R + 1 warped source copies are never stored (csrc/motion_encode.hip);
  * every 3x3 convolution, the nearest-x2 + 3x3 of an UpBlock2d (as 4 output phases of 2x2 taps: pack.upconv_w_kn_phases) and the 7x7
    output convolutions run through dawn_conv_gemm; eval-mode BatchNorm is folded to a / b in fp64 (flow_decoder._bn_ab); torch.cat of a
    decoder level and its skip is the conv's two-source input, never a tensor.
Channel counts that dawn_conv_gemm cannot take (3, 6, 44, 8, 10, 12 ...) are padded to the next multiple of 16 AT PACK TIME with zero
weights, zero bias and a = b = 0, so that padded channels are exact zeros throughout; `pad_conv_weight` is the one definition of that."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F_

from .flow_decoder import _bn_ab
from .pack import pack_bf3, pack_kn, upconv_w_kn_phases

Tensor = torch.Tensor


def pad16(n: int) -> int:
    return (n + 15) // 16 * 16


def pad_conv_weight(w: Tensor, segs: Sequence[Tuple[int, int]], n_pad: int) -> Tensor:
    """Conv2d weight (Co, Ci, kh, kw) whose Ci input channels are the concatenation of segments of `real` channels, each held in a buffer of
    `padded` channels: -> (n_pad, sum padded, kh, kw), zero at every padded input channel and every output channel past Co."""
    Co, Ci = w.shape[:2]
    if sum(r for r, _ in segs) != Ci or any(p < r for r, p in segs) or n_pad < Co:
        raise ValueError(f"pad_conv_weight: segments {list(segs)} do not cover {Ci} input channels, or {n_pad} < {Co} outputs")
    parts, o = [], 0
    for real, padded in segs:
        parts.append(F_.pad(w[:, o:o + real], (0, 0, 0, 0, 0, padded - real)))
        o += real
    return F_.pad(torch.cat(parts, 1), (0, 0, 0, 0, 0, 0, 0, n_pad - Co))


def unpad_conv_weight(wp: Tensor, segs: Sequence[Tuple[int, int]], n: int) -> Tensor:
    """The inverse of pad_conv_weight."""
    parts, o = [], 0
    for real, padded in segs:
        parts.append(wp[:n, o:o + real])
        o += padded
    return torch.cat(parts, 1)


def _pad_vec(v: Tensor, n: int) -> Tensor:
    return F_.pad(v.float(), (0, n - v.shape[0]))


@dataclass
class _Conv:
    w: Tensor                      # pack_kn image (mode 1: the four phase blocks)
    ws: Optional[Tensor]           # pack_bf3 image of a 3x3 / stride-1 conv
    bias: Optional[Tensor]
    N: int                         # padded output channels
    k: int = 3
    a: Optional[Tensor] = None     # the BatchNorm that follows
    b: Optional[Tensor] = None


def _pack(sd, prefix: str, segs, dev, norm: Optional[str] = None, up: bool = False, bias: bool = True, n_pad: Optional[int] = None) -> _Conv:
    w = sd[prefix + ".weight"].float()
    Co, k = w.shape[0], w.shape[2]
    N = pad16(Co) if n_pad is None else n_pad
    wp = pad_conv_weight(w, segs, N)
    if up:
        ph = upconv_w_kn_phases(wp.unsqueeze(2))
        c = _Conv(torch.stack([pack_kn(ph[i]) for i in range(4)], 0).to(dev), None, None, N, k)
    else:
        kn = wp.permute(2, 3, 1, 0).reshape(-1, N)
        c = _Conv(pack_kn(kn).to(dev), pack_bf3(kn).to(dev) if k == 3 else None, None, N, k)
    if bias:
        c.bias = _pad_vec(sd[prefix + ".bias"], N).to(dev).contiguous()
    if norm is not None:
        a, b = _bn_ab(sd, norm, "cpu")
        c.a, c.b = _pad_vec(a, N).to(dev).contiguous(), _pad_vec(b, N).to(dev).contiguous()
    return c


def _count(sd, stem: str) -> int:
    n = 0
    while f"{stem}.{n}.conv.weight" in sd:
        n += 1
    return n


class _Encoder:
    """UTIL:153-172 on rows: DownBlock2d = conv3x3 -> BN -> ReLU -> AvgPool 2x2.  `first_segs`: the input's channel segments."""

    def __init__(self, sd, stem: str, first_segs, dev, first_bias: bool = True):
        self.downs: List[_Conv] = []
        self.reals: List[int] = []                 # real (unpadded) output channels of every block: what ctx.motion_cfg states
        segs = list(first_segs)
        for i in range(_count(sd, stem)):
            p = f"{stem}.{i}"
            self.downs.append(_pack(sd, p + ".conv", segs, dev, norm=p + ".norm", bias=first_bias or i > 0))
            co = int(sd[p + ".conv.weight"].shape[0])
            self.reals.append(co)
            segs = [(co, pad16(co))]
        self.out_real = segs[0][0]


class _Hourglass:
    """UTIL:202-214 on rows; forward -> (last decoder level, input): the two sources of the 7x7 conv that follows (UTIL:198)."""

    def __init__(self, sd, prefix: str, in_real: int, dev):
        self.enc = _Encoder(sd, prefix + ".encoder.down_blocks", [(in_real, pad16(in_real))], dev)
        reals = [in_real] + [sd[f"{prefix}.encoder.down_blocks.{i}.conv.weight"].shape[0] for i in range(len(self.enc.downs))]
        self.ups: List[_Conv] = []
        self.up_reals: List[int] = []
        n = len(self.enc.downs)
        if _count(sd, prefix + ".decoder.up_blocks") != n or n == 0:
            raise ValueError(f"{prefix}: an Hourglass with as many up blocks as down blocks (at least one) is required")
        prev = None
        for j in range(n):
            p = f"{prefix}.decoder.up_blocks.{j}"
            skip = reals[n - j]
            segs = [(skip, pad16(skip))] if prev is None else [(prev, pad16(prev)), (skip, pad16(skip))]
            self.ups.append(_pack(sd, p + ".conv", segs, dev, norm=p + ".norm", up=True))
            prev = int(sd[p + ".conv.weight"].shape[0])
            self.up_reals.append(prev)
        self.out_segs = [(prev, pad16(prev)), (in_real, pad16(in_real))]
        self.levels = n

    def forward(self, ops, x: Tensor, F: int, h: int, w: int) -> Tuple[Tensor, Tensor]:
        if h % (1 << self.levels) or w % (1 << self.levels):
            raise ValueError(f"motion encode: the {h} x {w} map is not divisible by 2^{self.levels} (the Hourglass's skip sizes would not match)")
        outs, cur = [x], x
        for d in self.enc.downs:
            z = ops.conv_gemm(cur, d.w, d.N, F=F, Hi=h, Wi=w, KH=3, KW=3, stride=1, pad=1, bias=d.bias, w_bf3=d.ws)
            cur = ops.bn_relu_pool2(z, d.a, d.b, F, h, w)
            h, w = h // 2, w // 2
            outs.append(cur)
        out, skip = outs.pop(), None
        for u in self.ups:
            y = ops.conv_gemm(out, u.w, u.N, F=F, Hi=h, Wi=w, Ho=2 * h, Wo=2 * w, KH=2, KW=2, mode=1, in1=skip, bias=u.bias)
            h, w = 2 * h, 2 * w
            out = ops.affine_act(y, u.a, u.b, 1)
            skip = outs.pop()
        return out, skip


class MotionEncoder:
    """HIP-native LFG encode half.  `ops` is injectable (tests/motion_cases.MotionRefOps checks packing and orchestration on the CPU);
    the default HipOps raises if libdawn_hip.so is missing."""

    def __init__(self, generator_sd: Dict[str, Tensor], region_sd: Dict[str, Tensor], bg_sd: Dict[str, Tensor], device, ops=None,
                 chunk: int = 16, temperature: float = 0.1):
        gen = {k: torch.as_tensor(v) for k, v in generator_sd.items()}
        rp = {k: torch.as_tensor(v) for k, v in region_sd.items()}
        bg = {k: torch.as_tensor(v) for k, v in bg_sd.items()}
        if ops is None:
            from .ops import HipOps
            ops = HipOps()
        self.ops, self.device, self.chunk, self.temperature = ops, torch.device(device), int(chunk), float(temperature)
        dev = self.device
        pf = "pixelwise_flow_predictor"
        # ---- the shipped configuration, read off the checkpoints; everything else is refused
        if "jacobian.weight" in rp:
            raise ValueError("MotionEncoder: region_predictor has a `jacobian` conv (estimate_affine without pca_based); only pca_based=True is built")
        if "regions.weight" not in rp or "down.weight" not in rp:
            raise ValueError("MotionEncoder: region_predictor needs `regions` and a `down` buffer (scale_factor != 1; 0.25 is shipped)")
        if f"{pf}.mask.weight" not in gen:
            raise ValueError("MotionEncoder: the generator has no pixelwise_flow_predictor")
        if f"{pf}.occlusion.weight" not in gen:
            raise ValueError("MotionEncoder: estimate_occlusion_map=False is not built (the latent's third plane is the occlusion map)")
        if f"{pf}.down.weight" not in gen:
            raise ValueError("MotionEncoder: the pixelwise predictor needs a `down` buffer (scale_factor != 1; 0.25 is shipped)")
        if "fc.weight" not in bg or bg["fc.weight"].shape[0] != 6:
            raise ValueError("MotionEncoder: bg_predictor must be bg_type='affine' (fc with 6 outputs); 'zero', 'shift' and 'perspective' are not built")
        self.R = int(rp["regions.weight"].shape[0])
        if not 1 <= self.R <= 15:
            raise ValueError(f"MotionEncoder: num_regions = {self.R}: 1 .. 15 (10 is shipped)")
        k_rp, k_pf = int(rp["down.weight"].shape[-1]), int(gen[f"{pf}.down.weight"].shape[-1])
        if k_rp != k_pf or (k_rp - 1) % 4 != 0:
            raise ValueError(f"MotionEncoder: both predictors must share one integer 1 / scale_factor (antialias kernels of {k_rp} and {k_pf} taps)")
        self.s = (k_rp - 1) // 4 + 1
        cin_pf = int(gen[f"{pf}.hourglass.encoder.down_blocks.0.conv.weight"].shape[1])
        if cin_pf != (self.R + 1) * 4:
            raise ValueError(f"MotionEncoder: the pixelwise hourglass takes {cin_pf} channels, (num_regions + 1) * 4 = {(self.R + 1) * 4} are "
                             "built (use_deformed_source=True, 3 colour channels)")
        if int(mask_out := gen[f"{pf}.mask.weight"].shape[0]) != self.R + 1:
            raise ValueError(f"MotionEncoder: the mask conv has {mask_out} outputs, num_regions + 1 = {self.R + 1} expected")
        # ---- region predictor
        self.rp_hg = _Hourglass(rp, "predictor", 3, dev)
        self.rp_regions = _pack(rp, "regions", self.rp_hg.out_segs, dev)
        # ---- background encoder: the first conv split into its source half (with the bias, once per clip) and its driving half
        w0 = bg["encoder.down_blocks.0.conv.weight"].float()
        if w0.shape[1] != 6:
            raise ValueError("MotionEncoder: the background encoder takes the 6 channels of (source, driving)")
        self.bg_enc = _Encoder(bg, "encoder.down_blocks", [(3, 16), (3, 16)], dev)
        half = {"s.weight": w0[:, :3], "d.weight": w0[:, 3:], "s.bias": bg["encoder.down_blocks.0.conv.bias"]}
        self.bg_src0 = _pack(half, "s", [(3, 16)], dev)
        self.bg_drv0 = _pack(half, "d", [(3, 16)], dev, bias=False)
        self.bg_drv0.a, self.bg_drv0.b = self.bg_enc.downs[0].a, self.bg_enc.downs[0].b
        c_last = self.bg_enc.out_real
        self.fc_w = F_.pad(bg["fc.weight"].float(), (0, pad16(c_last) - c_last)).to(dev).contiguous()
        self.fc_b = bg["fc.bias"].float().to(dev).contiguous()
        # ---- pixelwise flow predictor: `mask` and `occlusion` as one 7x7 conv
        self.c_in_pf = pad16(cin_pf)
        self.pf_hg = _Hourglass(gen, f"{pf}.hourglass", cin_pf, dev)
        both = {"mo.weight": torch.cat((gen[f"{pf}.mask.weight"].float(), gen[f"{pf}.occlusion.weight"].float()), 0),
                "mo.bias": torch.cat((gen[f"{pf}.mask.bias"].float(), gen[f"{pf}.occlusion.bias"].float()), 0)}
        self.pf_out = _pack(both, "mo", self.pf_hg.out_segs, dev)
        self._bg_rep: Optional[Tensor] = None
        self._c_eval = None

    @classmethod
    def from_state_dicts(cls, generator_sd, region_sd, bg_sd, device, **kw) -> "MotionEncoder":
        return cls(generator_sd, region_sd, bg_sd, device, **kw)

    @classmethod
    def from_modules(cls, generator, region_predictor, bg_predictor, device=None, **kw) -> "MotionEncoder":
        """Build from the reference's (unchanged) modules: their state_dicts, and their attributes for what a state_dict cannot say."""
        pf = getattr(generator, "pixelwise_flow_predictor", None)
        want = [(region_predictor, "pca_based", True), (region_predictor, "scale_factor", 0.25), (pf, "scale_factor", 0.25),
                (pf, "use_deformed_source", True), (pf, "use_covar_heatmap", True), (pf, "revert_axis_swap", True),
                (bg_predictor, "bg_type", "affine")]
        for mod, name, value in want:
            if mod is None or getattr(mod, name, value) != value:
                raise ValueError(f"MotionEncoder: {name} = {getattr(mod, name, None)!r}; only the shipped configuration ({name} = {value!r}) is built")
        sd = generator.state_dict()
        if device is None:
            device = next(iter(sd.values())).device
        kw.setdefault("temperature", float(getattr(region_predictor, "temperature", 0.1)))
        return cls(sd, region_predictor.state_dict(), bg_predictor.state_dict(), device, **kw)

    # ------------------------------------------------------------------ pieces
    def _conv7(self, c: _Conv, pair: Tuple[Tensor, Tensor], F: int, h: int, w: int) -> Tensor:
        return self.ops.conv_gemm(pair[0], c.w, c.N, F=F, Hi=h, Wi=w, KH=7, KW=7, stride=1, pad=3, in1=pair[1], bias=c.bias)

    def _regions(self, down: Tensor, F: int, h: int, w: int):
        x = self._conv7(self.rp_regions, self.rp_hg.forward(self.ops, down, F, h, w), F, h, w)
        return self.ops.region_moments(x, F, h, w, self.R, self.temperature)

    def _frames(self, t: Tensor, what: str) -> Tensor:
        """fp32 (T,3,H,W) / (3,T,H,W)-permuted views with dense planes, or uint8 (T,H,W,3): as the op takes them."""
        if t.dtype == torch.uint8:
            if t.dim() != 4 or t.shape[3] != 3:
                raise ValueError(f"{what}: uint8 frames are (T,H,W,3)")
            return t.contiguous()
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"{what}: fp32 frames are (T,3,H,W)")
        t = t.float()
        return t if (t.stride(3) == 1 and t.stride(2) == t.shape[3]) else t.contiguous()

    @staticmethod
    def _size(t: Tensor) -> Tuple[int, int]:
        return (int(t.shape[1]), int(t.shape[2])) if t.dtype == torch.uint8 else (int(t.shape[2]), int(t.shape[3]))

    @torch.no_grad()
    def _encode(self, source_img: Tensor, driving: Tensor, grid: Tensor, conf: Tensor, chunk: Optional[int], conf_x0: bool) -> None:
        ops = self.ops
        src = self._frames(source_img if source_img.dim() == 4 else source_img.unsqueeze(0), "source_img")
        drv = self._frames(driving, "driving")
        if src.shape[0] != 1 or self._size(src) != self._size(drv):
            raise ValueError("motion encode: one source image of the driving frames' size is required")
        H, W = self._size(drv)
        T = int(drv.shape[0])
        h, w = -(-H // self.s), -(-W // self.s)
        nb = len(self.bg_enc.downs)
        if H % (1 << nb) or W % (1 << nb):
            raise ValueError(f"motion encode: the {H} x {W} frames are not divisible by 2^{nb} (the background encoder's pooling)")
        chunk = max(1, min(int(chunk or self.chunk), T))
        # ---- once per clip: the source's downsampled image, region parameters, and half of the background encoder's first conv
        src_down = ops.antialias_down(src, self.s, 16)
        s_shift, s_covar, s_affine = self._regions(src_down, 1, h, w)
        src_p = (s_shift[0], s_covar[0], s_affine[0])
        src_full = ops.antialias_down(src, 1, 16)
        c0 = self.bg_src0
        bg_src = ops.conv_gemm(src_full, c0.w, c0.N, F=1, Hi=H, Wi=W, KH=3, KW=3, stride=1, pad=1, bias=c0.bias, w_bf3=c0.ws)
        bg_rep = bg_src.unsqueeze(0).expand(chunk, H * W, c0.N).reshape(chunk * H * W, c0.N)        # the residual rows of a chunk's first conv
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            n = t1 - t0
            fr = drv[t0:t1]
            drv_p = self._regions(ops.antialias_down(fr, self.s, 16), n, h, w)
            d0 = self.bg_drv0
            z = ops.conv_gemm(ops.antialias_down(fr, 1, 16), d0.w, d0.N, F=n, Hi=H, Wi=W, KH=3, KW=3, stride=1, pad=1, res=bg_rep[:n * H * W],
                              w_bf3=d0.ws)
            cur, Hc, Wc = ops.bn_relu_pool2(z, d0.a, d0.b, n, H, W), H // 2, W // 2
            for d in self.bg_enc.downs[1:]:
                z = ops.conv_gemm(cur, d.w, d.N, F=n, Hi=Hc, Wi=Wc, KH=3, KW=3, stride=1, pad=1, bias=d.bias, w_bf3=d.ws)
                cur, Hc, Wc = ops.bn_relu_pool2(z, d.a, d.b, n, Hc, Wc), Hc // 2, Wc // 2
            bg = ops.bg_params(cur, n, self.fc_w, self.fc_b)
            rows = ops.motion_inputs(drv_p, src_p, bg, src_down, n, h, w, self.c_in_pf)
            x = self._conv7(self.pf_out, self.pf_hg.forward(ops, rows, n, h, w), n, h, w)
            ops.flow_combine(x, drv_p, src_p, bg, n, h, w, grid[:, t0:t1], conf[t0:t1], conf_x0)

    # ------------------------------------------------------------------ public
    def latent_size(self, H: int, W: int) -> Tuple[int, int]:
        return -(-H // self.s), -(-W // self.s)

    def c_evaluator(self):
        """The C-side stage of this encoder (ctx.MotionEvaluator), created on first use."""
        if self._c_eval is None:
            from .ctx import MotionEvaluator
            self._c_eval = MotionEvaluator(self)
        return self._c_eval

    def encode_clip(self, source_img: Tensor, driving: Tensor, chunk: Optional[int] = None, via_c: bool = False) -> Dict[str, Tensor]:
        """source_img (3,H,W) / (1,3,H,W) fp32 in [0,1] or (1,H,W,3) uint8; driving (T,3,H,W) fp32 -- a (3,T,H,W) clip permuted is taken
        without a copy -- or (T,H,W,3) uint8 -> {real_vid_grid (1,2,T,h,w), real_vid_conf (1,1,T,h,w)}, FD:259-260.
        via_c: the same launches from dawn_motion_encode_clip (csrc/dawn_motion.hip through ctx.MotionEvaluator), the same bits; driving
        may then also be I420 frames, (T, 3*H*W/2) uint8, converted chunk by chunk on the device.  The default path is unchanged."""
        if via_c:
            return self.c_evaluator().encode_clip(source_img, driving, chunk or self.chunk)
        T = int(driving.shape[0])
        h, w = self.latent_size(*self._size(self._frames(driving, "driving")))
        grid = torch.empty(2, T, h, w, device=driving.device, dtype=torch.float32)
        conf = torch.empty(T, h, w, device=driving.device, dtype=torch.float32)
        self._encode(source_img, driving, grid, conf, chunk, False)
        return {"real_vid_grid": grid.unsqueeze(0), "real_vid_conf": conf.view(1, 1, T, h, w)}

    def latent(self, source_img: Tensor, driving: Tensor, chunk: Optional[int] = None, via_c: bool = False) -> Tensor:
        """-> (3,T,h,w): the diffusion's x0 of this clip, cat(grid, 2 * conf - 1) (FD:280-282).  via_c: as encode_clip."""
        if via_c:
            return self.c_evaluator().latent(source_img, driving, chunk or self.chunk)
        T = int(driving.shape[0])
        h, w = self.latent_size(*self._size(self._frames(driving, "driving")))
        lat = torch.empty(3, T, h, w, device=driving.device, dtype=torch.float32)
        self._encode(source_img, driving, lat[:2], lat[2], chunk, True)
        return lat
