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

from .sampler import (CLIP_DEFAULT, KnownFrames, ancestral_step_scalars, chunk_plan, clip_mode, cosine_schedule_buffers, ddim_sample_clip,
                      ddim_step_scalars, dpmpp_step_scalars, draws_noise, known_level_scalars)

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
               noises: Optional[Sequence[Tensor]] = None, trace: bool = False, comm=None, known_latent: Optional[Tensor] = None,
               known_mask: Optional[Tensor] = None, known_noises: Optional[Sequence[Optional[Tensor]]] = None):
        """fea (B,256,h,w), bbox_mask (B,16,h,w), cond (B,T,1032) -> (B,3,T,h,w)   (MT:1137-1153).

        Extra keyword-only hooks (not in the reference): `x_init` / `noises` inject the random draws of
        MT:1166 / MT:1201 for parity tests; `comm` = T-shard communicator (cond then holds this rank's
        frames only).
        Known-frame conditioning (not in the reference; defined in include/dawn_hip.h, quality on a trained checkpoint unmeasured):
        `known_latent` (B,3,T,h,w) with `known_mask` (T,) or (B,T), nonzero = known, pins those frames -- the latent entering every
        step holds them at that step's noise level and the result holds them bit for bit; the other frames are generated to fit.
        `known_noises` (hook): S + 1 tensors (B,3,T,h,w), the noise of every level (the last, b = 0, may be None); default: the
        counter-based generator.  With `comm` both hold this rank's frames."""
        batch_size = cond.shape[0] if cond is not None else batch_size
        fea = torch.cat([fea, bbox_mask], dim=1)                                     # MT:1151
        shape = (batch_size, self.channels, self.num_frames, fea.shape[-1], fea.shape[-1])
        sample_fn = self.ddim_sample if self.is_ddim_sampling else self.p_sample_loop  # MT:1150
        return sample_fn(fea, shape, cond=cond, cond_scale=cond_scale, x_init=x_init, noises=noises, trace=trace, comm=comm,
                         known_latent=known_latent, known_mask=known_mask, known_noises=known_noises)

    @torch.inference_mode()
    def p_sample_loop(self, fea, shape, cond=None, cond_scale=1., *, x_init=None, noises=None, trace=False, comm=None,
                      known_latent=None, known_mask=None, known_noises=None):
        """The ancestral loop (MT:1124-1135): `num_timesteps` evaluations at t = num_timesteps-1 ... 0, whatever
        sampling_timesteps is.  noises[i] (hook) is read only for steps with t > 0, so num_timesteps - 1 entries suffice."""
        return self._sample_loop("ancestral", fea, shape, cond, cond_scale, x_init, noises, trace, comm, self.clip,
                                 (known_latent, known_mask, known_noises))

    @torch.no_grad()
    def ddim_sample(self, fea, shape, cond=None, cond_scale=1., clip_denoised=True, *, x_init=None, noises=None,
                    trace=False, comm=None, known_latent=None, known_mask=None, known_noises=None):
        """clip_denoised=False (MT:1183): x0 is used as predicted, neither thresholded nor clamped."""
        return self._sample_loop("ddim", fea, shape, cond, cond_scale, x_init, noises, trace, comm,
                                 self.clip if clip_denoised else ("none", None), (known_latent, known_mask, known_noises))

    def _known_frames(self, known, b, steps, kind, shape, device, seed):
        """sampler.KnownFrames of batch element b from the known_latent / known_mask / known_noises keywords, or None."""
        latent, mask, kz = known
        if latent is None:
            if mask is not None or kz is not None:
                raise ValueError("known_mask / known_noises need known_latent")
            return None
        if mask is None:
            raise ValueError("known_latent needs known_mask")
        B, C, T, h, w = shape
        if tuple(latent.shape) != (B, 3, T, h, w):
            raise ValueError(f"known_latent must be (B, 3, T, h, w) = {(B, 3, T, h, w)}, got {tuple(latent.shape)}")
        if mask.dim() == 1:
            mask = mask[None].expand(B, -1)
        if tuple(mask.shape) != (B, T):
            raise ValueError(f"known_mask must be (T,) or (B, T) with T = {T}, got {tuple(mask.shape)}")
        levels = known_level_scalars({k: getattr(self, k) for k in ("alphas_cumprod", "alphas_cumprod_prev")}, steps,
                                     "dpmpp" if self.solver == "dpmpp2m" else kind, self.num_timesteps)
        if kz is not None and len(kz) < len(levels) - 1:
            raise ValueError(f"known_noises: {len(levels)} entries needed (one per level; the last may be None), got {len(kz)}")
        noise_fn = None if kz is None else (lambda i: kz[i][b].contiguous().float().to(device))
        return KnownFrames((latent[b].contiguous().float().to(device)), (mask[b] != 0).to(torch.uint8).contiguous().to(device), levels,
                           noise_fn, seed)

    def _step_scalars(self, kind):
        """The per-step scalars of the loop `kind` under self.solver, from the schedule buffers."""
        bufs = {k: getattr(self, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                              "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped")}
        if kind == "ancestral":
            return ancestral_step_scalars(bufs, self.num_timesteps)
        if self.solver == "dpmpp2m":
            return dpmpp_step_scalars(bufs, self.sampling_timesteps, self.num_timesteps)
        return ddim_step_scalars(bufs, self.sampling_timesteps, self.ddim_sampling_eta, self.num_timesteps)

    def _sample_loop(self, kind, fea, shape, cond, cond_scale, x_init, noises, trace, comm, clip, known=(None, None, None)):
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
        steps = self._step_scalars(kind)
        step_kind = "dpmpp" if dpmpp else kind
        device = fea.device
        Ttotal, f0 = (T, 0) if comm is None else (comm.Ttotal, comm.f0)
        if cond is not None and cond.shape[1] != T:
            raise ValueError(f"cond has {cond.shape[1]} frames but num_frames={T}; call update_num_frames first (UVG:370)")
        seed = self.noise_seed

        def initial_latent(b):
            if x_init is not None:
                return x_init[b].contiguous().float()
            if seed is not None:
                return ops.philox_normal(3, T, f0, Ttotal, h * w, seed + b, 0, device).reshape(3, T, h, w)
            return torch.randn(3, T, h, w, device=device)                             # MT:1166

        def known_seed(s):
            """The seed of the known-frame noise: `s`, or unseeded (and no known_noises given) ONE draw from the global generator."""
            if known[0] is not None and s is None and known[2] is None:
                s = int(torch.randint(0, 2 ** 62, (1,)).item())
            return s

        outs, traces = [], []
        if self.use_ctx and comm is None and not trace and fea.is_cuda:
            ev = unet.ctx_evaluator()
            rcos, rsin = P.rotary_tables(T + 2 * P.win)
            for b in range(B):
                clip_mem = ev.prepare_clip(fea[b].contiguous().float(), cond[b].contiguous().float(), rcos, rsin)
                null_clip = ev.prepare_null_clip(fea[b].contiguous().float(), T, rcos, rsin) if cond_scale != 1.0 else None
                x0 = initial_latent(b)
                nz = None
                if noises is not None:
                    nz = [noises[i][b].contiguous() if draws_noise(step_kind, st) else None for i, st in enumerate(steps)]
                run_seed = (seed + b) if seed is not None else None
                if nz is None and run_seed is None and not dpmpp:
                    # unseeded (MT:1201 draws from the global generator): ONE draw from it seeds the evaluator's counter-based
                    # generator -- S x 3 x T x h x w floats of pre-drawn noise would be GBs for the long clips the path supports
                    run_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
                run_seed = known_seed(run_seed)
                kw = dict(null_clip=null_clip, cond_scale=cond_scale, x0_clip=None if clip == CLIP_DEFAULT else clip,
                          known=self._known_frames(known, b, steps, kind, shape, device, run_seed or 0))
                if not dpmpp:
                    kw.update(seed=run_seed or 0, noises=nz)
                run = ev.sample_dpmpp if dpmpp else ev.sample_ancestral if ancestral else ev.sample
                outs.append(run(clip_mem, x0, steps, **kw))
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

            def noise_fn(i, b=b):
                if noises is not None:
                    return noises[i][b].contiguous()
                if seed is not None:
                    return ops.philox_normal(3, T, f0, Ttotal, h * w, seed + b, i + 1, device).reshape(3, T, h, w)
                return torch.randn(3, T, h, w, device=device)                         # MT:1201

            x0 = initial_latent(b)
            tr = [] if trace else None
            kf = self._known_frames(known, b, steps, kind, shape, device, known_seed(seed + b if seed is not None else None) or 0)
            outs.append(ddim_sample_clip(ops, P, cs, x0, steps, noise_fn, cond_scale, cs_null, tr, use_graph=self.use_graph,
                                         eager_every=self.eager_every, kind=step_kind, clip=clip, known=kf))
            traces.append(tr)
        self.last_trace = traces if trace else None
        self.last_route = "python"
        return torch.stack(outs, 0)

    # ------------------------------------------------------------------ chunked generation of a long clip (not in the reference)
    def iter_chunks(self, fea, bbox_mask, cond, cond_scale=1., *, chunk_frames: int, overlap: int, comm=None):
        """Sample a clip of T = cond.shape[1] frames as the chunks of sampler.chunk_plan(T, chunk_frames, overlap), yielding
        (first_frame, latent (B,3,n,h,w)) as each chunk finishes -- the frames it emits, in order, so a host can decode and show them
        while the next chunk samples.  Chunk j runs `sample` on the cond rows of its frames with the previous chunk's overlapping
        frames as its known set (known_latent / known_mask over its first known_j frames) and the seed noise_seed + (j << 32)
        (unseeded: the global generator, as always).  The cond rows are those of the whole clip, computed once by the caller, so
        init_pose / init_eye stay anchored to frame 0.  Every chunk has one shape (one workspace, one clip_mem size, one graph).
        An overlapping frame is bit-identical in both chunks that hold it.  Whether a seam shows or the motion drifts on a trained
        checkpoint, and which overlap is enough, has not been measured.  T-shard (comm) cannot be combined with chunking."""
        if comm is not None:
            raise ValueError("chunked sampling cannot be combined with a T-shard (comm): shard the whole clip, or chunk it on one GPU")
        if cond is None:
            raise ValueError("chunked sampling needs cond (B, T, cond_dim): its length is the clip's")
        plan = chunk_plan(int(cond.shape[1]), int(chunk_frames), int(overlap))      # (refusals raise here, not at the first next())
        return self._chunks(plan, fea, bbox_mask, cond, cond_scale)

    def _chunks(self, plan, fea, bbox_mask, cond, cond_scale):
        prev, prev_start = None, 0
        for j, (start, n, kn) in enumerate(plan):
            kl = km = None
            if kn:
                kl = torch.zeros_like(prev)
                kl[:, :, :kn] = prev[:, :, start - prev_start:start - prev_start + kn]
                km = torch.zeros(n, dtype=torch.uint8, device=prev.device)
                km[:kn] = 1
            saved = (self.num_frames, getattr(self.denoise_fn, "num_frames", None), self.noise_seed)
            try:
                self.num_frames = n
                if saved[1] is not None:
                    self.denoise_fn.num_frames = n
                if saved[2] is not None:
                    self.noise_seed = saved[2] + (j << 32)
                out = self.sample(fea, bbox_mask, cond=cond[:, start:start + n].contiguous(), cond_scale=cond_scale, known_latent=kl,
                                  known_mask=km)
            finally:
                self.num_frames, self.noise_seed = saved[0], saved[2]
                if saved[1] is not None:
                    self.denoise_fn.num_frames = saved[1]
            prev, prev_start = out, start
            yield start + kn, out[:, :, kn:]

    def sample_chunked(self, fea, bbox_mask, cond, cond_scale=1., *, chunk_frames: int, overlap: int, comm=None):
        """The whole clip (B,3,T,h,w) from iter_chunks: the emitted frames concatenated."""
        return torch.cat([lat for _, lat in self.iter_chunks(fea, bbox_mask, cond, cond_scale, chunk_frames=chunk_frames, overlap=overlap,
                                                              comm=comm)], dim=2)

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
