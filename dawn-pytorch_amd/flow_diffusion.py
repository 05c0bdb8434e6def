"""`FlowDiffusion`: the inference wrapper contract of SURVEY.md §8b B1(iii)
(FD = DM_3/modules/video_flow_diffusion_model_multiGPU_v0_crema_vgg_floss_plus_faceemb_flow_fast_init_cond_test.py,
FD:96-201, 325-406): owns `.generator` (the LFG flow generator, injected: the reference's unchanged module or a
`FlowDecoder`), `.unet`, `.diffusion`, `.face_loc_emb`; `update_num_frames`, `generate_bbox_mask`,
`sample_one_video` keep the reference's signatures and semantics.  The denoising hot path
(`self.diffusion.sample`) runs on the HIP kernels, and so does the flow decode that follows it (SURVEY §8f N1:
`flow_decoder.FlowDecoder`, built from the injected generator's state_dict, replaces the reference's per-frame
`forward_with_flow` loop FD:372-385 when the clip lives on the GPU).  The few lines of tensor algebra around them
(condition assembly, bbox rasterisation, the 2-conv `Face_loc_Encoder`) are once-per-clip host-side plumbing and
stay in torch by default, device-agnostic (the reference hard-codes `.cuda()`); with `inputs_via_c = True` a GPU clip of
one sample takes them from the C-side clip-input stage instead (`ctx.InputsEvaluator`: dawn_clip_inputs, what a host
without Python calls).
"""
from __future__ import annotations

import time
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F_

from .diffusion import DynamicNfGaussianDiffusion
from .flow_decoder import FlowDecoder
from .motion_encoder import MotionEncoder
from .unet import DynamicNfUnet3D


class Face_loc_Encoder(nn.Module):
    """FD:39-50: bbox mask (B,1,H,W) -> (B,16,H/4,W/4)."""

    def __init__(self, dim=1):
        super().__init__()
        self.conv1 = nn.Conv2d(dim, 8, kernel_size=3, stride=2, padding=1)
        self.conv2 = nn.Conv2d(8, 16, kernel_size=3, stride=2, padding=1)

    def forward(self, x):
        return F_.relu(self.conv2(F_.relu(self.conv1(x))))


def load_reference_lfg(config_pth: str, pretrained_pth: str, device):
    """Build the reference's own (unchanged) LFG generator when its package is importable (FD:112-122)."""
    import yaml
    try:
        from LFG.modules.generator import Generator          # the reference repo must be on PYTHONPATH
    except Exception as e:                                    # pragma: no cover - depends on user environment
        raise RuntimeError("FlowDiffusion needs the unchanged LFG generator: pass `generator=` or put the DAWN "
                           "reference repo (LFG/) on PYTHONPATH") from e
    ckpt = torch.load(pretrained_pth, map_location=device)
    with open(config_pth) as f:
        cfg = yaml.safe_load(f)
    gen = Generator(num_regions=cfg['model_params']['num_regions'], num_channels=cfg['model_params']['num_channels'],
                    revert_axis_swap=cfg['model_params']['revert_axis_swap'],
                    **cfg['model_params']['generator_params']).to(device)
    gen.load_state_dict(ckpt['generator'])
    gen.eval()
    for p in gen.parameters():
        p.requires_grad = False
    return gen


class FlowDiffusion(nn.Module):
    def __init__(self, img_size=32, num_frames=40, sampling_timesteps=250, win_width=40, null_cond_prob=0.1,
                 ddim_sampling_eta=1., pose_dim=7, dim_mults=(1, 2, 4, 8), is_train=True, use_residual_flow=False,
                 learn_null_cond=False, use_deconv=True, padding_mode="zeros", pretrained_pth=None, config_pth=None,
                 generator=None, device=None, native_decode: Optional[bool] = None, region_predictor=None, bg_predictor=None,
                 motion_encoder: Optional[MotionEncoder] = None):
        """`region_predictor`, `bg_predictor` (the reference's unchanged modules, beside its `generator` module) or a ready `motion_encoder`:
        the LFG's encode half, needed by `encode_video` / `reenact` only (FD:124-136 loads them from the same checkpoint).
        `native_decode`: True = decode on the HIP kernels (error without a GPU / the extension), False = call the
        injected generator's `forward_with_flow` frame by frame exactly like FD:375-383, None (default) = HIP kernels
        whenever the clip is on the GPU."""
        super().__init__()
        if use_residual_flow:
            raise NotImplementedError("use_residual_flow=True is not used by the shipped configs")
        self.use_residual_flow = use_residual_flow
        if generator is None:
            generator = load_reference_lfg(config_pth, pretrained_pth, device or "cuda")
        self.generator = generator
        self.native_decode = native_decode
        self._decoder: Optional[FlowDecoder] = generator if isinstance(generator, FlowDecoder) else None
        self.region_predictor, self.bg_predictor, self._motion = region_predictor, bg_predictor, motion_encoder
        self.pose_dim = pose_dim
        self.unet = DynamicNfUnet3D(dim=64, cond_dim=1024 + pose_dim + 2, cond_aud=1024, cond_pose=pose_dim,
                                    cond_eye=2, num_frames=num_frames, channels=3 + 256 + 16, out_grid_dim=2,
                                    out_conf_dim=1, dim_mults=dim_mults, use_hubert_audio_cond=True,
                                    learn_null_cond=learn_null_cond, use_final_activation=False,
                                    use_deconv=use_deconv, padding_mode=padding_mode, win_width=win_width)
        self.diffusion = DynamicNfGaussianDiffusion(denoise_fn=self.unet, num_frames=num_frames, image_size=img_size,
                                                    sampling_timesteps=sampling_timesteps, timesteps=1000,
                                                    loss_type='l2', use_dynamic_thres=True,
                                                    null_cond_prob=null_cond_prob,
                                                    ddim_sampling_eta=ddim_sampling_eta)
        self.face_loc_emb = Face_loc_Encoder()
        self.is_train = is_train        # kept for signature parity; this build is inference-only
        self.inputs_via_c = False       # True: bbox_mask and cond of a GPU clip with B == 1 from dawn_clip_inputs (ctx.InputsEvaluator)
        self._inputs_ev = None
        self.motion_via_c = False       # True: encode_video / reenact encode a GPU clip with B == 1 through dawn_motion_encode_clip (ctx.MotionEvaluator)
        # chunked sampling of a long clip (not in the reference; GaussianDiffusion.sample_chunked): plain attributes like diffusion.solver.
        # chunk_frames = None: the clip is sampled whole, as always
        self.chunk_frames: Optional[int] = None
        self.chunk_overlap = 0

    def update_num_frames(self, new_num_frames):
        """FD:177-180."""
        self.unet.update_num_frames(new_num_frames)
        self.diffusion.update_num_frames(new_num_frames)

    def flow_decoder(self, device) -> FlowDecoder:
        """The HIP decoder for the injected generator (weights packed once, on first use)."""
        if self._decoder is None:
            self._decoder = FlowDecoder.from_generator(self.generator, device)
        return self._decoder

    def motion_encoder(self, device) -> MotionEncoder:
        """The HIP encode half (weights packed once, on first use)."""
        if self._motion is None:
            if self.region_predictor is None or self.bg_predictor is None or not hasattr(self.generator, "state_dict"):
                raise ValueError("encode_video / reenact need the LFG's encode half: pass motion_encoder=, or region_predictor= and "
                                 "bg_predictor= beside the reference's generator module")
            self._motion = MotionEncoder.from_modules(self.generator, self.region_predictor, self.bg_predictor, device)
        return self._motion

    def decodes_natively(self, sample_img) -> bool:
        """Does sample_one_video decode this clip with `FlowDecoder` (rather than frame by frame through the injected generator)?"""
        native = self.native_decode
        if native is None:
            native = sample_img.is_cuda and (self._decoder is not None or hasattr(self.generator, "state_dict"))
        return bool(native)

    def generate_bbox_mask(self, bbox, size=32):
        """FD:182-201.  bbox (B,6,1) = [x_min,x_max,y_min,y_max,H,W].  Unlike the reference this does not
        rescale the caller's tensor in place and indexes with int32 (the reference's uint8 indices wrap
        for size > 256)."""
        b = bbox[:, :, 0].clone().float()
        b[:, :2] = (b[:, :2] / b[:, 4].unsqueeze(1)) * size
        b[:, 2:4] = (b[:, 2:4] / b[:, 5].unsqueeze(1)) * size
        lt = b[:, :4:2].to(torch.int32)
        rb = (b[:, 1:4:2] + 1).to(torch.int32)
        n = b.shape[0]
        rows = torch.arange(size, device=b.device, dtype=torch.int32).view(1, size, 1).expand(n, size, size)
        cols = torch.arange(size, device=b.device, dtype=torch.int32).view(1, 1, size).expand(n, size, size)
        mask = (rows >= lt[:, 1].view(n, 1, 1)) & (rows <= rb[:, 1].view(n, 1, 1)) & \
               (cols >= lt[:, 0].view(n, 1, 1)) & (cols <= rb[:, 0].view(n, 1, 1))
        return mask.unsqueeze(1).float()

    def assemble_cond(self, sample_audio_hubert, sample_pose, sample_eye, init_pose=None, init_eye=None):
        """FD:332-350: cond = cat[hubert, pose - init_pose, eye - init_eye] -> (B, T, 1024 + pose_dim + 2)."""
        sample_pose = sample_pose[:, :self.pose_dim]
        ref_pose = sample_pose.permute(0, 2, 1)
        ref_eye = sample_eye.permute(0, 2, 1)
        T = ref_pose.shape[1]
        ip = ref_pose[:, 0] if init_pose is None else init_pose
        ip = ip.unsqueeze(1).repeat(1, T, 1)[:, :, :self.pose_dim]
        ie = ref_eye[:, 0] if init_eye is None else init_eye
        ie = ie.unsqueeze(1).repeat(1, ref_eye.shape[1], 1)
        if ref_pose.shape[-1] != ip.shape[-1]:
            ref_pose = torch.cat([ref_pose, ip[:, :, -1].unsqueeze(-1)], dim=-1)
        return torch.cat([sample_audio_hubert, ref_pose - ip, ref_eye - ie], dim=-1)

    def clip_inputs(self, sample_img, sample_audio_hubert, sample_pose, sample_eye, sample_bbox, init_pose=None, init_eye=None):
        """(bbox_mask (B,16,h,w), cond (B,T,cond_dim)) of FD:327-350: the torch plumbing, or -- `inputs_via_c`, a GPU clip, B == 1 --
        the C-side stage.  The evaluator holds pointers into `face_loc_emb`'s parameters: it is rebuilt when they moved."""
        if not (self.inputs_via_c and sample_img.is_cuda and sample_img.shape[0] == 1):
            return (self.face_loc_emb(self.generate_bbox_mask(sample_bbox, size=sample_img.shape[-1])),
                    self.assemble_cond(sample_audio_hubert, sample_pose, sample_eye, init_pose, init_eye))
        from .ctx import InputsEvaluator
        key = tuple(p.data_ptr() for p in self.face_loc_emb.parameters())
        if self._inputs_ev is None or self._inputs_ev[0] != key:
            self._inputs_ev = (key, InputsEvaluator(self, n_aud=sample_audio_hubert.shape[-1]))
        pose = sample_pose[0, :self.pose_dim].t().float().contiguous()      # (T, n_pose) rows, as assemble_cond permutes them
        eye = sample_eye[0].t().float().contiguous()
        size = sample_img.shape[-1]
        fea16 = torch.empty(16, size // 4, size // 4, device=sample_img.device)
        cond = self._inputs_ev[1].clip_inputs(sample_bbox[0, :, 0].tolist(), size, fea16, sample_audio_hubert[0].float().contiguous(), pose, eye,
                                             None if init_pose is None else init_pose[0, :self.pose_dim].tolist(),
                                             None if init_eye is None else init_eye[0].tolist())
        return fea16.unsqueeze(0), cond.unsqueeze(0)

    def _decode_bytes(self, sample_img, grid, conf, frames_u8: dict):
        """The `frames_u8` options of sample_one_video / reenact on a latent: -> (output key, the byte tensor or the chunk generator)."""
        kw = dict(frames_u8)
        stream = kw.pop("stream", False)
        fmt = kw.pop("format", "rgb")
        if fmt not in ("rgb", "yuv420p"):
            raise ValueError(f"frames_u8 format must be 'rgb' or 'yuv420p', not {fmt!r}")
        if fmt == "yuv420p" and kw.pop("bgr", False):
            raise ValueError("frames_u8 format='yuv420p' has no channel order: bgr=True is not allowed")
        dec = self.flow_decoder(sample_img.device)
        if stream and sample_img.shape[0] != 1:
            raise ValueError("frames_u8 stream=True takes one clip (B == 1)")
        if fmt == "yuv420p":
            fn = dec.stream_frames_yuv420 if stream else dec.decode_clip_yuv420
            return "sample_frames_yuv420", fn(sample_img, grid, conf, **kw)
        fn = dec.stream_frames_u8 if stream else dec.decode_clip_u8
        return "sample_frames_u8", fn(sample_img, grid, conf, **kw)

    def _encode(self, ref_img, real_vid):
        """ref_img (B,3,H,W), real_vid (B,3,T,H,W) fp32 in [0,1] -- or, B == 1, (T,H,W,3) uint8 frames -> grid (B,2,T,h,w), conf (B,1,T,h,w).
        `motion_via_c` (a GPU clip, B == 1): the C-side stage, which also takes I420 frames, (T, 3*H*W/2) uint8."""
        me = self.motion_encoder(ref_img.device)
        via_c = bool(self.motion_via_c) and ref_img.is_cuda and ref_img.shape[0] == 1
        if real_vid.dtype == torch.uint8 and real_vid.dim() == 2 and not via_c:
            raise ValueError("I420 driving frames (T, 3*H*W/2) need motion_via_c = True, a GPU clip and B == 1")
        if real_vid.dtype == torch.uint8:
            if ref_img.shape[0] != 1:
                raise ValueError("uint8 driving frames take one clip (B == 1)")
            clips = [me.encode_clip(ref_img[0], real_vid, via_c=via_c)]
        else:
            clips = [me.encode_clip(ref_img[b], real_vid[b].permute(1, 0, 2, 3), via_c=via_c) for b in range(ref_img.shape[0])]
        return torch.cat([c["real_vid_grid"] for c in clips], 0), torch.cat([c["real_vid_conf"] for c in clips], 0)

    @torch.no_grad()
    def encode_video(self, ref_img, real_vid):
        """What FlowDiffusion.forward computes under no_grad from a real clip (FD:248-262), with the reference's keys: real_vid_grid
        (B,2,T,h,w), real_vid_conf (B,1,T,h,w) from the HIP encode half (`MotionEncoder`), real_out_vid / real_warped_vid (B,3,T,H,W) from
        the batched `FlowDecoder` on that latent."""
        grid, conf = self._encode(ref_img, real_vid)
        dec = self.flow_decoder(ref_img.device).decode_clip(ref_img, grid, conf)
        return {"real_vid_grid": grid, "real_vid_conf": conf, "real_out_vid": dec["sample_out_vid"], "real_warped_vid": dec["sample_warped_vid"]}

    @torch.no_grad()
    def reenact(self, sample_img, driving, frames_u8: Optional[dict] = None):
        """Video-driven reenactment, the LFG's own use: the motion of `driving` ((B,3,T,H,W) fp32, or (T,H,W,3) uint8 frames for one
        clip, or with `motion_via_c` its I420 bytes (T, 3*H*W/2) uint8) encoded against `sample_img` (B,3,H,W) and decoded from it.  -> real_vid_grid, real_vid_conf, and sample_out_vid /
        sample_warped_vid -- or, with `frames_u8` (the options of sample_one_video: RGB or format="yuv420p", stream or not),
        sample_frames_u8 / sample_frames_yuv420 instead."""
        grid, conf = self._encode(sample_img, driving)
        out = {"real_vid_grid": grid, "real_vid_conf": conf}
        if frames_u8 is not None:
            key, frames = self._decode_bytes(sample_img, grid, conf, frames_u8)
            out[key] = frames
            return out
        out.update(self.flow_decoder(sample_img.device).decode_clip(sample_img, grid, conf))
        return out

    @torch.no_grad()
    def sample_one_video(self, sample_img, sample_audio_hubert, sample_pose, sample_eye, sample_bbox, cond_scale,
                         init_pose=None, init_eye=None, real_vid=None, frames_u8: Optional[dict] = None):
        """FD:325-406.  `frames_u8` (not in the reference): None = the fp32 clips as always; dict(mean=(0,0,0), bgr=False, chunk=None,
        stream=False) = decode straight to bytes instead (native decode only): out["sample_frames_u8"] is the (B,T,H,W,3) uint8
        device tensor of FlowDecoder.decode_clip_u8 -- or, with stream=True (B == 1), the chunk generator of
        FlowDecoder.stream_frames_u8 -- and "sample_out_vid" / "sample_warped_vid" are never materialised.  dict(format="yuv420p",
        mean=, chunk=, stream=) decodes to planar YUV 4:2:0 instead (format defaults to "rgb"): out["sample_frames_yuv420"] is the
        (B,T,3HW/2) uint8 tensor of FlowDecoder.decode_clip_yuv420, or the generator of stream_frames_yuv420; it has no bgr."""
        out = {}
        fea = self.generator.compute_fea(sample_img)                                   # (B,256,h,w)  GEN:132-136
        bbox_mask, cond = self.clip_inputs(sample_img, sample_audio_hubert, sample_pose, sample_eye, sample_bbox, init_pose, init_eye)
        t0 = time.time()
        if self.chunk_frames is not None:     # cond rows of the whole clip (init_pose / init_eye anchored to frame 0), sampled chunk by chunk
            pred = self.diffusion.sample_chunked(fea, bbox_mask, cond, cond_scale, chunk_frames=self.chunk_frames, overlap=self.chunk_overlap)
        else:
            pred = self.diffusion.sample(fea, bbox_mask, cond=cond, batch_size=fea.size(0), cond_scale=cond_scale)
        out["sample_vid_grid"] = pred[:, :2]
        out["sample_vid_conf"] = (pred[:, 2].unsqueeze(1) + 1) * 0.5
        out["ddim_seconds"] = time.time() - t0
        native = self.decodes_natively(sample_img)
        if frames_u8 is not None:
            if not native:
                raise ValueError("sample_one_video(frames_u8=...) needs the native flow decode (native_decode, or a clip on the GPU)")
            key, frames = self._decode_bytes(sample_img, out["sample_vid_grid"], out["sample_vid_conf"], frames_u8)
            out[key] = frames
            return out
        if native:                                                                     # FD:372-385 as one batched decode
            out.update(self.flow_decoder(sample_img.device).decode_clip(sample_img, out["sample_vid_grid"],
                                                                        out["sample_vid_conf"]))
            return out
        frames, warped = [], []
        for idx in range(pred.size(2)):                                                # FD:375-383 (unchanged LFG)
            g = self.generator.forward_with_flow(source_image=sample_img,
                                                 optical_flow=out["sample_vid_grid"][:, :, idx].permute(0, 2, 3, 1),
                                                 occlusion_map=out["sample_vid_conf"][:, :, idx])
            frames.append(g["prediction"])
            warped.append(g["deformed"])
        out["sample_out_vid"] = torch.stack(frames, dim=2)
        out["sample_warped_vid"] = torch.stack(warped, dim=2)
        return out
