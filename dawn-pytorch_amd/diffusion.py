"""`GaussianDiffusion` / `DynamicNfGaussianDiffusion`: the sampler contract of SURVEY.md §8b B1(ii)
(`diffusion.sample(fea, bbox_mask, cond=..., batch_size, cond_scale)`, MT:1137-1153 -> `ddim_sample`
MT:1156-1208) on the HIP op set.  Same constructor signature and the same 12 schedule buffers in the
`state_dict` as the reference (MT:988-1055), so `model.diffusion.load_state_dict(ckpt['diffusion'])`
(UVG:527-528) works unchanged.  `sample` dispatches as the reference does (MT:1150): DDIM when sampling_timesteps <
timesteps, else the ancestral loop `p_sample_loop` (MT:1113-1135).  x0 is clipped as the reference clips it (MT:1094-1107,
MT:1183-1196): `use_dynamic_thres=True` -> dynamic thresholding at `dynamic_thres_percentile` (the shipped pipeline: 0.9, FD:164),
`use_dynamic_thres=False` (the constructor default) -> static clamp to [-1, 1], `ddim_sample(clip_denoised=False)` -> none.
Not in the reference: `solver = "dpmpp2m"` (a plain attribute, default "ddim") runs DPM-Solver++(2M) on the DDIM time grid instead of
the DDIM update, on every host; its definition is in include/dawn_hip.h.  Quality against the number of steps on a trained checkpoint
has not been measured.
Inference only: the training losses (MT:1226-1281) are out of scope."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import nn

from .sampler import (CLIP_DEFAULT, ancestral_sample_clip, ancestral_step_scalars, clip_mode, cosine_schedule_buffers, ddim_sample_clip,
                      ddim_step_scalars, dpmpp_sample_clip, dpmpp_step_scalars)

Tensor = torch.Tensor


_ALLOC_SET = False
ALLOC_ENV = ("PYTORCH_HIP_ALLOC_CONF", "PYTORCH_CUDA_ALLOC_CONF", "PYTORCH_ALLOC_CONF")


def _long_clip_allocator(T: int, like: Tensor, environ=None) -> Optional[str]:
    """Long clips (the memory-lean form, unet_forward.LONG_CLIP_FRAMES) allocate tensors of many GB each: PyTorch's caching
    allocator then must not split its large blocks, or 20 % of HBM ends up reserved but unusable (56,000 frames failed with 55 GiB
    in fragments, profiles/r3_max_clip_length.log).  Applied here, ONCE per process, and ONLY when the user configured nothing:
    the setting is process-global and permanent, and the allocator's parser resets every option the string does not name -- so a
    caller who set PYTORCH_HIP_ALLOC_CONF / PYTORCH_CUDA_ALLOC_CONF / PYTORCH_ALLOC_CONF keeps exactly what they asked for (and
    should add `max_split_size_mb:2048` there themselves for clips this long: INTEGRATION.md).  Returns what was done (also
    logged once through `warnings`): "applied", "kept user configuration", "unavailable: ..." or None when nothing was needed."""
    global _ALLOC_SET
    import os
    import warnings
    from .unet_forward import LONG_CLIP_FRAMES
    if _ALLOC_SET or T <= LONG_CLIP_FRAMES or not like.is_cuda:
        return None
    _ALLOC_SET = True
    env = os.environ if environ is None else environ
    user = [k for k in ALLOC_ENV if env.get(k)]
    if user:
        warnings.warn(f"dawn_pytorch_amd: {T}-frame clip, caching-allocator configuration left as set by {user[0]} "
                      f"(add max_split_size_mb:2048 there for clips this long)", stacklevel=3)
        return "kept user configuration"
    try:
        torch.cuda.memory._set_allocator_settings("max_split_size_mb:2048")
    except (AttributeError, RuntimeError, ValueError) as e:      # (private API: an optimisation of the reachable length only)
        warnings.warn(f"dawn_pytorch_amd: could not set max_split_size_mb:2048 for a {T}-frame clip ({type(e).__name__}: {e})",
                      stacklevel=3)
        return f"unavailable: {type(e).__name__}"
    warnings.warn(f"dawn_pytorch_amd: {T}-frame clip -- caching allocator set to max_split_size_mb:2048 for this process "
                  f"(no PYTORCH_*_ALLOC_CONF in the environment)", stacklevel=3)
    return "applied"


class GaussianDiffusion(nn.Module):
    def __init__(self, denoise_fn, *, image_size, num_frames, text_use_bert_cls=False, channels=3, timesteps=1000,
                 sampling_timesteps=250, ddim_sampling_eta=1., loss_type='l1', use_dynamic_thres=False,
                 dynamic_thres_percentile=0.9, null_cond_prob=0.1):
        super().__init__()
        self.null_cond_prob = null_cond_prob
        self.channels = channels
        self.image_size = image_size
        self.num_frames = num_frames
        self.denoise_fn = denoise_fn
        for k, v in cosine_schedule_buffers(timesteps).items():
            self.register_buffer(k, v)
        self.num_timesteps = int(timesteps)
        self.loss_type = loss_type
        self.sampling_timesteps = sampling_timesteps if sampling_timesteps is not None else timesteps
        self.is_ddim_sampling = self.sampling_timesteps < timesteps
        self.ddim_sampling_eta = ddim_sampling_eta
        self.text_use_bert_cls = text_use_bert_cls
        self.use_dynamic_thres = use_dynamic_thres
        self.dynamic_thres_percentile = dynamic_thres_percentile
        # the x0 clipping mode every sampler path runs (sampler.clip_mode); a percentile outside [0, 1] raises ValueError here
        # (torch.quantile would at the first step)
        self.clip = clip_mode(("dynamic", dynamic_thres_percentile) if use_dynamic_thres else ("static",))
        # reproducibility knobs (the reference draws from the global torch generator)
        self.noise_seed: Optional[int] = None     # int -> shard-invariant Philox stream on device
        self.use_graph = False                    # capture one UNet evaluation per clip as a HIP graph
        self.eager_every = 0                      # with use_graph: run every n-th step eagerly (profiling hooks)
        self.use_ctx = False                      # run the sampler loop through the C-side evaluator (dawn_sampler_run, or
                                                  # dawn_sampler_run_guided when cond_scale != 1; dawn_sampler_run_ancestral for
                                                  # the ancestral loop; dawn_sampler_run_clip / _ancestral_clip for any clipping
                                                  # mode but dynamic at 0.9); same kernels and arguments as the Python
                                                  # orchestration: bit-identical output
        self.solver = "ddim"                      # "ddim": the reference's update; "dpmpp2m": DPM-Solver++(2M) on the same time pairs
                                                  # (needs sampling_timesteps < timesteps; deterministic after the initial
                                                  # latent: ddim_sampling_eta and `noises` are not read, noise_seed only seeds
                                                  # the initial latent).  A plain attribute: neither a constructor argument
                                                  # nor a buffer
        self.last_route: Optional[str] = None     # "ctx" or "python": which host ran the last sample()
        self.last_trace: Optional[list] = None

    # ------------------------------------------------------------------ reference call surface
    @torch.inference_mode()
    def sample(self, fea, bbox_mask, cond=None, cond_scale=1., batch_size=16, *, x_init: Optional[Tensor] = None,
               noises: Optional[Sequence[Tensor]] = None, trace: bool = False, comm=None):
        """fea (B,256,h,w), bbox_mask (B,16,h,w), cond (B,T,1032) -> (B,3,T,h,w)   (MT:1137-1153).

        Extra keyword-only hooks (not in the reference): `x_init` / `noises` inject the random draws of
        MT:1166 / MT:1201 for parity tests; `comm` = T-shard communicator (cond then holds this rank's
        frames only)."""
        batch_size = cond.shape[0] if cond is not None else batch_size
        fea = torch.cat([fea, bbox_mask], dim=1)                                     # MT:1151
        shape = (batch_size, self.channels, self.num_frames, fea.shape[-1], fea.shape[-1])
        sample_fn = self.ddim_sample if self.is_ddim_sampling else self.p_sample_loop  # MT:1150
        return sample_fn(fea, shape, cond=cond, cond_scale=cond_scale, x_init=x_init, noises=noises, trace=trace, comm=comm)

    @torch.inference_mode()
    def p_sample_loop(self, fea, shape, cond=None, cond_scale=1., *, x_init=None, noises=None, trace=False, comm=None):
        """The ancestral loop (MT:1124-1135): `num_timesteps` evaluations at t = num_timesteps-1 ... 0, whatever
        sampling_timesteps is.  noises[i] (hook) is read only for steps with t > 0, so num_timesteps - 1 entries suffice."""
        return self._sample_loop("ancestral", fea, shape, cond, cond_scale, x_init, noises, trace, comm, self.clip)

    @torch.no_grad()
    def ddim_sample(self, fea, shape, cond=None, cond_scale=1., clip_denoised=True, *, x_init=None, noises=None,
                    trace=False, comm=None):
        """clip_denoised=False (MT:1183): x0 is used as predicted, neither thresholded nor clamped."""
        return self._sample_loop("ddim", fea, shape, cond, cond_scale, x_init, noises, trace, comm,
                                 self.clip if clip_denoised else ("none", None))

    def _sample_loop(self, kind, fea, shape, cond, cond_scale, x_init, noises, trace, comm, clip):
        """One host loop for every sampler (kind "ddim" / "ancestral"; solver "dpmpp2m" turns "ddim" into the DPM-Solver++(2M) steps
        on the same time pairs): the C-side evaluator when use_ctx, else the Python orchestration; they share the evaluation and
        differ in the step scalars and the step tail.  clip = (kind, q) of sampler.clip_mode."""
        if self.solver not in ("ddim", "dpmpp2m"):
            raise ValueError(f'unknown solver {self.solver!r}: "ddim" or "dpmpp2m"')
        dpmpp = self.solver == "dpmpp2m"
        if dpmpp and (kind != "ddim" or not self.is_ddim_sampling):
            raise ValueError('solver = "dpmpp2m" runs on the DDIM time grid: it needs sampling_timesteps < timesteps')
        ancestral = kind == "ancestral"
        clip = clip_mode(clip, ancestral)
        unet = self.denoise_fn
        ops = unet._ops()
        if comm is not None:
            ops = ops.with_comm(comm)
        _long_clip_allocator(shape[2], fea)
        P = unet.packed()
        B, C, T, h, w = shape
        if ancestral:
            steps = ancestral_step_scalars({k: getattr(self, k) for k in (
                "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                "posterior_log_variance_clipped")}, self.num_timesteps)
        elif dpmpp:
            steps = dpmpp_step_scalars({k: getattr(self, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                                       "sqrt_recipm1_alphas_cumprod")}, self.sampling_timesteps,
                                       self.num_timesteps)
        else:
            S, eta = self.sampling_timesteps, self.ddim_sampling_eta
            steps = ddim_step_scalars({k: getattr(self, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                                      "sqrt_recipm1_alphas_cumprod")}, S, eta,
                                      self.num_timesteps)
        # steps that draw noise (MT:1120 / MT:1201); DPM-Solver++(2M) draws none
        noisy = [not dpmpp and (st["t"] > 0 if ancestral else st["t_next"] > 0) for st in steps]
        device = fea.device
        Ttotal, f0 = (T, 0) if comm is None else (comm.Ttotal, comm.f0)
        if cond is not None and cond.shape[1] != T:
            raise ValueError(f"cond has {cond.shape[1]} frames but num_frames={T}; call update_num_frames first (UVG:370)")
        outs, traces = [], []
        if self.use_ctx and comm is None and not trace and fea.is_cuda:
            ev = unet.ctx_evaluator()
            rcos, rsin = P.rotary_tables(T + 2 * P.win)
            for b in range(B):
                clip_mem = ev.prepare_clip(fea[b].contiguous().float(), cond[b].contiguous().float(), rcos, rsin)
                null_clip = ev.prepare_null_clip(fea[b].contiguous().float(), T, rcos, rsin) if cond_scale != 1.0 else None
                seed = self.noise_seed
                if x_init is not None:
                    x0 = x_init[b].contiguous().float()
                elif seed is not None:
                    x0 = ops.philox_normal(3, T, 0, T, h * w, seed + b, 0, device).reshape(3, T, h, w)
                else:
                    x0 = torch.randn(3, T, h, w, device=device)                       # MT:1166
                nz = None
                if noises is not None:
                    nz = [noises[i][b].contiguous() if noisy[i] else None for i in range(len(steps))]
                run_seed = (seed + b) if seed is not None else None
                if nz is None and run_seed is None and not dpmpp:
                    # unseeded (MT:1201 draws from the global generator): ONE draw from it seeds the evaluator's counter-based
                    # generator -- S x 3 x T x h x w floats of pre-drawn noise would be GBs for the long clips the path supports
                    run_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                x0_clip = None if clip == CLIP_DEFAULT else clip
                if dpmpp:
                    outs.append(ev.sample_dpmpp(clip_mem, x0, steps, null_clip=null_clip, cond_scale=cond_scale, x0_clip=x0_clip))
                    continue
                run = ev.sample_ancestral if ancestral else ev.sample
                outs.append(run(clip_mem, x0, steps, seed=run_seed or 0, noises=nz, null_clip=null_clip, cond_scale=cond_scale,
                                x0_clip=x0_clip))
            self.last_trace = None
            self.last_route = "ctx"
            return torch.stack(outs, 0)
        for b in range(B):
            cs = unet.build_clip(fea[b].contiguous().float(), cond[b].contiguous().float(), comm=comm,
                                 Ttotal=Ttotal, f0=f0)
            cs_null = None
            if cond_scale != 1.0:
                cs_null = unet.build_clip(fea[b].contiguous().float(), torch.zeros_like(cond[b]).float(), comm=comm,
                                          Ttotal=Ttotal, f0=f0)
            seed = self.noise_seed

            def noise_fn(i, b=b):
                if noises is not None:
                    return noises[i][b].contiguous()
                if seed is not None:
                    return ops.philox_normal(3, T, f0, Ttotal, h * w, seed + b, i + 1, device).reshape(3, T, h, w)
                return torch.randn(3, T, h, w, device=device)                         # MT:1201

            if x_init is not None:
                x0 = x_init[b].contiguous().float()
            elif seed is not None:
                x0 = ops.philox_normal(3, T, f0, Ttotal, h * w, seed + b, 0, device).reshape(3, T, h, w)
            else:
                x0 = torch.randn(3, T, h, w, device=device)                           # MT:1166
            tr = [] if trace else None
            if dpmpp:
                outs.append(dpmpp_sample_clip(ops, P, cs, x0, steps, cond_scale, cs_null, tr, use_graph=self.use_graph,
                                              eager_every=self.eager_every, clip=clip))
            else:
                outs.append((ancestral_sample_clip if ancestral else ddim_sample_clip)(
                    ops, P, cs, x0, steps, noise_fn, cond_scale, cs_null, tr, use_graph=self.use_graph, eager_every=self.eager_every,
                    clip=clip))
            traces.append(tr)
        self.last_trace = traces if trace else None
        self.last_route = "python"
        return torch.stack(outs, 0)

    def forward(self, *a, **k):
        raise NotImplementedError("training (p_losses, MT:1234-1281) is out of scope of the HIP inference build")


class DynamicNfGaussianDiffusion(GaussianDiffusion):
    """MT:1307-1313."""

    def __init__(self, default_num_frames=20, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.default_num_frames = default_num_frames
        self.num_frames = default_num_frames

    def update_num_frames(self, new_num_frames):
        self.num_frames = new_num_frames
