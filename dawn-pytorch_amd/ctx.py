"""Python binding of the C-side evaluator (include/dawn_hip.h: dawn_ctx_* / dawn_clip_prepare / dawn_unet_forward /
dawn_sampler_run(_ancestral); csrc/dawn_ctx.hip) -- what a non-Python host would call, used here by the tests (bit-identical to the
Python orchestration of unet_forward.py / sampler.py) and optionally by the sampler (`GaussianDiffusion.use_ctx`).  `DecoderEvaluator`,
`HubertEvaluator`, `PbnetEvaluator` and `InputsEvaluator` below bind the flow decoder, the HuBERT stage, the PBnet pose / blink stage and
the clip-input stage the same way; the five share `_Evaluator` (weight table, handle, stream, workspace).  Every entry is bound once, in _lib.lib().

PyTorch only provides device memory (the packed weights, the per-clip table memory, the workspace) and the stream."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .pack import PackedAttn, PackedResBlock, PackedUNet

Tensor = torch.Tensor


class UnetCfg(C.Structure):
    """Mirror of ``dawn_unet_cfg``."""
    _fields_ = [("dim", C.c_int), ("n_levels", C.c_int), ("dim_mults", C.c_int * 8), ("fea_ch", C.c_int),
                ("cond_aud", C.c_int), ("cond_pose", C.c_int), ("cond_eye", C.c_int), ("win", C.c_int)]


class NamedPtr(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ptr", C.c_void_p)]


class DdimStep(C.Structure):
    """Mirror of ``dawn_ddim_step``."""
    _fields_ = [("t", C.c_int), ("t_next", C.c_int), ("recip", C.c_float), ("recipm1", C.c_float),
                ("sqrt_alpha_next", C.c_float), ("c", C.c_float), ("sigma", C.c_float)]


class AncestralStep(C.Structure):
    """Mirror of ``dawn_ancestral_step``."""
    _fields_ = [("t", C.c_int), ("recip", C.c_float), ("recipm1", C.c_float), ("c1", C.c_float), ("c2", C.c_float),
                ("std", C.c_float)]


class DpmppStep(C.Structure):
    """Mirror of ``dawn_dpmpp_step``."""
    _fields_ = [("t", C.c_int), ("recip", C.c_float), ("recipm1", C.c_float), ("a", C.c_float), ("b", C.c_float), ("c", C.c_float)]


class ClipMode(C.Structure):
    """Mirror of ``dawn_clip_mode``."""
    _fields_ = [("kind", C.c_int), ("q", C.c_double)]


CLIP_KINDS = {"dynamic": 0, "static": 1, "none": 2}      # DAWN_CLIP_DYNAMIC / _STATIC / _NONE
SOLVER_DDIM, SOLVER_ANCESTRAL, SOLVER_DPMPP = 0, 1, 2    # DAWN_SOLVER_DDIM / _ANCESTRAL / _DPMPP


# CtxEvaluator method -> (solver tag, mirror of its step struct, sampler.draws_noise kind)
_SOLVERS = {"sample": (SOLVER_DDIM, DdimStep, "ddim"), "sample_ancestral": (SOLVER_ANCESTRAL, AncestralStep, "ancestral"),
            "sample_dpmpp": (SOLVER_DPMPP, DpmppStep, "dpmpp")}
# solver tag -> its entry when (x0_clip is given, guided, sharded, none of these); CtxEvaluator._entry
_ENTRIES = {SOLVER_DDIM: ("dawn_sampler_run_clip", "dawn_sampler_run_guided", "dawn_sampler_run_sharded", "dawn_sampler_run"),
            SOLVER_ANCESTRAL: ("dawn_sampler_run_ancestral_clip",) + ("dawn_sampler_run_ancestral",) * 3,
            SOLVER_DPMPP: ("dawn_sampler_run_dpmpp",) * 4}
_NO_CLIP_MODE = ("dawn_sampler_run", "dawn_sampler_run_sharded", "dawn_sampler_run_guided", "dawn_sampler_run_ancestral")


def _clip_struct(clip, ancestral: bool) -> ClipMode:
    from .sampler import clip_mode
    kind, q = clip_mode(clip, ancestral)
    return ClipMode(CLIP_KINDS[kind], 0.0 if q is None else q)


# (values of OPT_CONV_POLICY / OPT_TEMPORAL_FLAGS: policy.ConvPolicy / policy.TemporalFlags)
OPT_CONV_POLICY, OPT_TEMPORAL_FLAGS, OPT_OVERLAP, OPT_PROFILE, OPT_LONG_CLIP_FRAMES, OPT_UP_BORDER, OPT_FOLD_HEADS = 1, 2, 3, 4, 5, 6, 7

# ---- T-shard callbacks (include/dawn_hip.h: dawn_shard_comm)
HALO_BEGIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.c_void_p)
HALO_END_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)


class ShardCommC(C.Structure):
    """Mirror of ``dawn_shard_comm``."""
    _fields_ = [("user", C.c_void_p), ("rank", C.c_int), ("world", C.c_int), ("halo_begin", HALO_BEGIN_FN),
                ("halo_end", HALO_END_FN), ("allreduce_sum_f64", ALLREDUCE_FN), ("allreduce_sum_u32", ALLREDUCE_FN),
                ("allreduce_min_u32", ALLREDUCE_FN)]


class ShardCallbacks:
    """Builds a ``dawn_shard_comm`` from five Python callables working on torch VIEWS of the evaluator's workspace (the buffers the C
    side hands to the callbacks live inside it):
        halo_begin(xe (Fext*HW, C) float32, hl, F, hh)   halo_end()   sum_f64(t)   sum_i32(t)   min_i32(t)
    `from_tshard(comm)` wires them to a tshard.TShardComm (torch.distributed: RCCL on GPUs)."""

    def __init__(self, rank: int, world: int, halo_begin, halo_end, sum_f64, sum_i32, min_i32):
        self.rank, self.world = rank, world
        self.fns = (halo_begin, halo_end, sum_f64, sum_i32, min_i32)
        self.ws: Optional[Tensor] = None         # set by CtxEvaluator before each sharded call
        self.frame_shape = None
        self.error: Optional[BaseException] = None

        def view(ptr, nbytes, dtype):
            off = ptr - self.ws.data_ptr()
            if off < 0 or off + nbytes > self.ws.numel():
                raise _lib.DawnHipError("shard callback: buffer outside the evaluator's workspace")
            return self.ws[off:off + nbytes].view(dtype)

        def guard(f):
            def g(*a):
                try:
                    f(*a)
                    return 0
                except BaseException as e:       # noqa: BLE001  (must not propagate through the C frames)
                    self.error = e
                    return -213
            return g

        def hb(user, xe, hl, F, hh, frame_floats, stream):
            t = view(xe, (hl + F + hh) * frame_floats * 4, torch.float32)
            halo_begin(t, hl, F, hh, frame_floats)

        def he(user, stream):
            halo_end()

        def mk(fn, dtype, size):
            def cb(user, buf, n, stream):
                fn(view(buf, n * size, dtype))
            return cb

        self._keep = (HALO_BEGIN_FN(guard(hb)), HALO_END_FN(guard(he)), ALLREDUCE_FN(guard(mk(sum_f64, torch.float64, 8))),
                      ALLREDUCE_FN(guard(mk(sum_i32, torch.int32, 4))), ALLREDUCE_FN(guard(mk(min_i32, torch.int32, 4))))
        self.c = ShardCommC(None, rank, world, *self._keep)

    @staticmethod
    def from_tshard(comm, win: int) -> "ShardCallbacks":
        """comm: tshard.TShardComm; win: the model's temporal window (what each neighbour needs from this rank)."""
        comm.set_window(win)
        state = {}

        def hb(xe, hl, F, hh, frame_floats):
            state["works"], state["xe"] = comm.halo_post(xe, hl, F, hh, frame_floats), xe

        def he():
            comm.wait_works(state.pop("works", []), state.pop("xe", None))     # (timed when comm.timing is on, like the Python rank's)

        return ShardCallbacks(comm.rank, comm.world, hb, he, comm.all_reduce_sum, comm.all_reduce_sum, comm.all_reduce_min)


def named_weights(P: PackedUNet) -> Dict[str, Tensor]:
    """PackedUNet -> {dotted name: device tensor} in the naming scheme of include/dawn_hip.h."""
    out: Dict[str, Tensor] = {}

    def put(k, t):
        if t is not None:
            out[k] = t

    def attn(p: str, a: PackedAttn):
        for f in ("wqkv", "wout", "bout", "wqkv_s", "wout_s", "wout_sp"):
            put(p + f, getattr(a, f))

    def rb(p: str, r: PackedResBlock):
        for f in ("w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "wr", "br", "w1s", "w2s", "w1w", "w2w", "w1w4", "w2w4", "wrs", "wq", "wqs", "q_scale", "g3"):
            put(p + f, getattr(r, f))
        for f in ("wo", "wos", "mlp_w", "mlp_b", "kv_w", "k_scale", "null_kv"):
            lst = getattr(r, f)
            if lst is not None:
                for b, t in enumerate(lst):
                    put(f"{p}{f}.{b}", t)

    for f in ("w3", "wfea", "b_init", "rel_emb", "sin_freqs", "t_w1", "t_b1", "t_w2", "t_b2", "film_w", "film_b", "wg", "bg",
              "wo", "bo"):
        put(f, getattr(P, f))
    put("rot_freqs", P.rot_freqs.detach().float().contiguous().to(P.rel_emb.device))
    attn("init_tattn.", P.init_tattn)
    for l, lvl in enumerate(P.downs):
        rb(f"downs.{l}.rb1.", lvl["rb1"]); rb(f"downs.{l}.rb2.", lvl["rb2"])
        attn(f"downs.{l}.sla.", lvl["sla"]); attn(f"downs.{l}.tattn.", lvl["tattn"])
        if lvl["down"] is not None:
            put(f"downs.{l}.down.w", lvl["down"][0]); put(f"downs.{l}.down.b", lvl["down"][1])
            if lvl["down"][2] is not None:
                put(f"downs.{l}.down.ws", lvl["down"][2])
    rb("mid.rb1.", P.mid["rb1"]); rb("mid.rb2.", P.mid["rb2"])
    attn("mid.sattn.", P.mid["sattn"]); attn("mid.tattn.", P.mid["tattn"])
    for l, lvl in enumerate(P.ups):
        rb(f"ups.{l}.rb1.", lvl["rb1"]); rb(f"ups.{l}.rb2.", lvl["rb2"])
        attn(f"ups.{l}.sla.", lvl["sla"]); attn(f"ups.{l}.tattn.", lvl["tattn"])
        if lvl["up"] is not None:
            put(f"ups.{l}.up.w", lvl["up"][0]); put(f"ups.{l}.up.b", lvl["up"][1])
            if lvl["up"][2] is not None:
                put(f"ups.{l}.up.ws", lvl["up"][2])
    rb("head_g.", P.head_g); rb("head_o.", P.head_o)
    return out


class _Evaluator:
    """What the five C-side handles share: the library, the named-pointer table of `weights` (kept alive: the handle holds raw
    pointers), creation and destruction, the caller's stream and one grow-only workspace."""

    def __init__(self, create_name: str, destroy_name: str, cfg: C.Structure, weights: Dict[str, Tensor], device, fp32_only: bool):
        """fp32_only: every table entry must be fp32 (the UNet and decoder tables carry split bf16 images as well)."""
        self.L = _lib.lib()
        self.device, self.cfg, self.weights, self._destroy = device, cfg, weights, destroy_name
        arr = (NamedPtr * max(1, len(weights)))()
        self._names = [k.encode() for k in weights]
        for i, (k, t) in enumerate(weights.items()):
            if not t.is_cuda or not t.is_contiguous() or (fp32_only and t.dtype != torch.float32):
                raise _lib.DawnHipError(f"packed weight {k} must be a contiguous {'fp32 ' if fp32_only else ''}GPU tensor")
            arr[i].name, arr[i].ptr = self._names[i], t.data_ptr()
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(getattr(self.L, create_name)(C.addressof(cfg), C.addressof(arr), len(weights), C.addressof(h)), create_name)
        self.h = h
        self._ws: Optional[Tensor] = None

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            getattr(self.L, self._destroy)(h)

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def _grown(self, nbytes: int) -> Tensor:
        """The evaluator's own workspace, at least `nbytes` long; it only ever grows.  0 is a size query's refusal."""
        if nbytes <= 0:
            raise _lib.DawnHipError(f"no workspace size: {self.L.dawn_last_error().decode()}")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None              # (the old one goes first)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws


class CtxEvaluator(_Evaluator):
    """One `dawn_ctx` for one packed model on one device."""

    def __init__(self, P: PackedUNet):
        self.P = P
        cfg = UnetCfg()
        cfg.dim, cfg.n_levels = P.dim, P.n_levels
        for i in range(P.n_levels):
            cfg.dim_mults[i] = P.dims[i + 1] // P.dim
        cfg.fea_ch = P.fea_ch
        cfg.cond_aud, cfg.cond_pose, cfg.cond_eye = P.cond_dims
        cfg.win = P.win
        super().__init__("dawn_ctx_create", "dawn_ctx_destroy", cfg, named_weights(P), P.rel_emb.device, fp32_only=False)
        self._need = {}              # (F, h, w, conv policy) -> dawn_workspace_bytes (a dry evaluation on the host: cached)
        self._policy = 0
        if P.up_border:              # folded up convs (use_deconv=False): what their outside taps read
            self.set_option(OPT_UP_BORDER, P.up_border)
        if os.environ.get("DAWN_FOLD_HEADS", "1") == "0":      # (the A/B switch HipOps.fold_heads reads: both hosts follow it)
            self.set_option(OPT_FOLD_HEADS, 0)

    def set_option(self, option: int, value: int) -> None:
        check(self.L.dawn_ctx_set_option(self.h, option, int(value)), "dawn_ctx_set_option")
        if option == OPT_CONV_POLICY:
            self._policy = int(value)
        if option != OPT_PROFILE:
            self._need.clear()              # kernel-family options change the launch sequence, hence the requirement

    def workspace(self, F: int, h: int, w: int, shard: Optional[ShardCallbacks] = None, guided: bool = False) -> Tensor:
        key = (F, h, w, self._policy, None if shard is None else (shard.rank, shard.world))
        if guided:
            key = key + ("guided",)
        need = self._need.get(key)
        if need is None:                    # sized in C for both schedules (one / two streams)
            if guided:
                rank, world = (0, 1) if shard is None else (shard.rank, shard.world)
                need = self._need[key] = int(self.L.dawn_workspace_bytes_guided(self.h, F, h, w, rank, world))
            else:
                need = self._need[key] = int(self.L.dawn_workspace_bytes(self.h, F, h, w) if shard is None else
                                             self.L.dawn_workspace_bytes_sharded(self.h, F, h, w, shard.rank, shard.world))
        return self._grown(need)

    def prepare_clip(self, fea272: Tensor, cond: Tensor, rcos: Optional[Tensor] = None, rsin: Optional[Tensor] = None) -> dict:
        """fea272 (fea_ch, h, w), cond (F, cond_dim) -> the per-clip table memory (a dict holding the buffer + shape)."""
        Cf, h, w = fea272.shape
        F = cond.shape[0]
        if not (fea272.is_cuda and fea272.is_contiguous() and cond.is_cuda and cond.stride(1) == 1 and fea272.dtype == torch.float32
                and cond.dtype == torch.float32):
            raise _lib.DawnHipError("prepare_clip: fea272 must be a contiguous fp32 GPU tensor, cond an fp32 GPU tensor with unit column stride")
        mem = torch.empty(int(self.L.dawn_clip_bytes(self.h, F, h, w)), dtype=torch.uint8, device=self.device)
        ws = self.workspace(F, h, w)
        check(self.L.dawn_clip_prepare(self.h, F, h, w, fea272.data_ptr(), cond.data_ptr(), cond.stride(0),
                                       None if rcos is None else rcos.data_ptr(), None if rsin is None else rsin.data_ptr(),
                                       mem.data_ptr(), mem.numel(), ws.data_ptr(), ws.numel(), self._stream()), "dawn_clip_prepare")
        return {"mem": mem, "F": F, "h": h, "w": w}

    def prepare_null_clip(self, fea272: Tensor, F: int, rcos: Optional[Tensor] = None, rsin: Optional[Tensor] = None) -> dict:
        """The clip of the all-zero condition (learn_null_cond=False, MT:920) for guided sampling: ONE zero row read with row stride 0."""
        cd = sum(self.P.cond_dims)
        zero = torch.zeros(1, cd, device=fea272.device, dtype=torch.float32).expand(F, cd)
        return self.prepare_clip(fea272, zero, rcos, rsin)

    def _shard_call(self, shard: ShardCallbacks, rc: int, what: str) -> None:
        err, shard.error = shard.error, None
        if err is not None:
            raise err
        check(rc, what)

    def forward(self, clip: dict, x3: Tensor, t: float, shard: Optional[ShardCallbacks] = None) -> Tensor:
        """shard: this evaluator runs ONE rank of a T-sharded clip (clip = this rank's frames), exchanging through the callbacks."""
        F, h, w = clip["F"], clip["h"], clip["w"]
        if not (x3.is_cuda and x3.is_contiguous() and tuple(x3.shape) == (3, F, h, w) and x3.dtype == torch.float32):
            raise _lib.DawnHipError(f"forward: x3 must be a contiguous fp32 GPU tensor of shape (3, {F}, {h}, {w})")
        out = torch.empty_like(x3)
        ws = self.workspace(F, h, w, shard)
        if shard is not None:
            shard.ws = ws
            self._shard_call(shard, self.L.dawn_unet_forward_sharded(self.h, F, h, w, clip["mem"].data_ptr(), x3.data_ptr(), float(t),
                                                                     out.data_ptr(), ws.data_ptr(), ws.numel(), C.addressof(shard.c),
                                                                     self._stream()), "dawn_unet_forward_sharded")
            return out
        check(self.L.dawn_unet_forward(self.h, F, h, w, clip["mem"].data_ptr(), x3.data_ptr(), float(t), out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), self._stream()), "dawn_unet_forward")
        return out

    def forward_guided(self, clip: dict, null_clip: dict, x3: Tensor, t: float, cond_scale: float,
                       shard: Optional[ShardCallbacks] = None) -> Tensor:
        """dawn_unet_forward_guided: null + (cond - null) * cond_scale, the condition-free prefix evaluated once."""
        F, h, w = clip["F"], clip["h"], clip["w"]
        if not (x3.is_cuda and x3.is_contiguous() and tuple(x3.shape) == (3, F, h, w) and x3.dtype == torch.float32):
            raise _lib.DawnHipError(f"forward_guided: x3 must be a contiguous fp32 GPU tensor of shape (3, {F}, {h}, {w})")
        out = torch.empty_like(x3)
        ws = self.workspace(F, h, w, shard, guided=True)
        comm = None
        if shard is not None:
            shard.ws = ws
            comm = C.addressof(shard.c)
        rc = self.L.dawn_unet_forward_guided(self.h, F, h, w, clip["mem"].data_ptr(), null_clip["mem"].data_ptr(), x3.data_ptr(), float(t),
                                             float(cond_scale), out.data_ptr(), ws.data_ptr(), ws.numel(), comm, self._stream())
        if shard is not None:
            self._shard_call(shard, rc, "dawn_unet_forward_guided")
        else:
            check(rc, "dawn_unet_forward_guided")
        return out

    def sample(self, clip: dict, x_init: Tensor, steps: Sequence[dict], seed: int = 0,
               noises: Optional[List[Optional[Tensor]]] = None, want_thresholds: bool = False,
               shard: Optional[ShardCallbacks] = None, null_clip: Optional[dict] = None, cond_scale: float = 1.0, x0_clip=None,
               known=None, known_entry: bool = False):
        """cond_scale != 1 (with null_clip = prepare_null_clip(...)): guided sampling, dawn_sampler_run_guided.
        noises[i] is read only for steps with t_next > 0, and must be there for those.
        known (sampler.KnownFrames): known-frame conditioning through dawn_sampler_run_known (every form: guided, sharded, any clipping
        mode); known_entry=True takes that entry without a known set too (bit-identical to the entries below).
        x0_clip (sampler.clip_mode; None: dynamic thresholding at 0.9 through the entries above): any x0 clipping mode through
        dawn_sampler_run_clip, single / guided / sharded alike.  Thresholds: static [1, 1] per step, none: rows left as allocated."""
        return self._run("sample", clip, x_init, steps, seed, noises, want_thresholds, shard, null_clip, cond_scale, x0_clip, known,
                         known_entry)

    def sample_ancestral(self, clip: dict, x_init: Tensor, steps: Sequence[dict], seed: int = 0,
                         noises: Optional[List[Optional[Tensor]]] = None, want_thresholds: bool = False,
                         shard: Optional[ShardCallbacks] = None, null_clip: Optional[dict] = None, cond_scale: float = 1.0,
                         x0_clip=None, known=None, known_entry: bool = False):
        """dawn_sampler_run_ancestral: the ancestral loop (sampler.ancestral_step_scalars), guided when cond_scale != 1 (null_clip =
        prepare_null_clip(...)), one T-shard rank when `shard` is given.  noises[i] is read only for steps with t > 0.
        x0_clip (sampler.clip_mode; None: dynamic thresholding at 0.9 through that entry): ("dynamic", q) or ("static",) through
        dawn_sampler_run_ancestral_clip.  known / known_entry: as for sample()."""
        return self._run("sample_ancestral", clip, x_init, steps, seed, noises, want_thresholds, shard, null_clip, cond_scale, x0_clip,
                         known, known_entry)

    def sample_dpmpp(self, clip: dict, x_init: Tensor, steps: Sequence[dict], want_thresholds: bool = False,
                     shard: Optional[ShardCallbacks] = None, null_clip: Optional[dict] = None, cond_scale: float = 1.0, x0_clip=None,
                     known=None, known_entry: bool = False):
        """dawn_sampler_run_dpmpp: the DPM-Solver++(2M) loop (sampler.dpmpp_step_scalars), guided when cond_scale != 1 (null_clip =
        prepare_null_clip(...)), one T-shard rank when `shard` is given.  Deterministic: no seed, no noises.  x0_clip (sampler.clip_mode;
        None: dynamic thresholding at 0.9): any clipping mode.  Thresholds: static [1, 1] per step, none: rows left as allocated.
        known / known_entry: as for sample() (the known-frame noise is the only noise this loop draws)."""
        return self._run("sample_dpmpp", clip, x_init, steps, 0, None, want_thresholds, shard, null_clip, cond_scale, x0_clip, known,
                         known_entry)

    @staticmethod
    def _entry(solver: int, known: bool, clipped: bool, guided: bool, sharded: bool) -> str:
        """The C entry a sampler method takes: the first column of its row that applies (known or known_entry, x0_clip given, guided,
        shard, neither).  Several entries reach one loop, and the GPU tests compare them: the choice is behaviour."""
        if known:
            return "dawn_sampler_run_known"
        return _ENTRIES[solver][0 if clipped else 1 if guided else 2 if sharded else 3]

    @staticmethod
    def _noise_ptrs(who: str, kind: str, steps: Sequence[dict], noises, n: int):
        """noises -> the `noises` array of the C entries: the tensor of every step that draws noise, NULL for the others (never read)."""
        from .sampler import draws_noise
        nz = (C.c_void_p * max(len(steps), 1))()
        for i, st in enumerate(steps):
            if not draws_noise(kind, st):
                continue
            t = noises[i] if i < len(noises) else None
            if t is None:                        # (the C loop would take NULL for "no noise" and return a wrong clip)
                raise _lib.DawnHipError(f"{who}: noises[{i}] missing for a step that draws noise (t = {st['t']})")
            if not (t.is_cuda and t.is_contiguous() and t.numel() == n and t.dtype == torch.float32):
                raise _lib.DawnHipError(f"{who}: noises[{i}] must be a contiguous fp32 GPU tensor of {n} elements")
            nz[i] = t.data_ptr()
        return nz

    @staticmethod
    def _sample_known(who: str, solver: int, known, S: int, F: int, n: int, seed: int, nz):
        """The known-set arguments of dawn_sampler_run_known (sampler.KnownFrames, or None: all NULL) and the seed the entry runs with:
        ((latent, mask, ab, known noises), seed, the tensors to keep alive over the call)."""
        if known is None:
            return (None, None, None, None), seed, []
        lat, msk, kz, keep = known.latent, known.mask, None, []
        if not (lat.is_cuda and lat.is_contiguous() and lat.dtype == torch.float32 and lat.numel() == n):
            raise _lib.DawnHipError(f"{who}: known.latent must be a contiguous fp32 GPU tensor of {n} elements")
        if not (msk.is_cuda and msk.is_contiguous() and msk.dtype == torch.uint8 and msk.numel() == F):
            raise _lib.DawnHipError(f"{who}: known.mask must be {F} uint8 values on the GPU")
        if len(known.levels) != S + 1:
            raise _lib.DawnHipError(f"{who}: known.levels must hold {S + 1} (a, b) pairs")
        ab = (C.c_float * (2 * (S + 1)))(*[float(v) for lv in known.levels for v in lv])
        if known.noise_fn is not None:
            kz = (C.c_void_p * (S + 1))()
            for i, (_, b) in enumerate(known.levels):
                z = known.noise_fn(i) if b != 0.0 else None
                if z is not None and not (z.is_cuda and z.is_contiguous() and z.dtype == torch.float32 and z.numel() == n):
                    raise _lib.DawnHipError(f"{who}: known noise {i} must be a contiguous fp32 GPU tensor of {n} elements")
                if z is None and b != 0.0:
                    raise _lib.DawnHipError(f"{who}: known noise {i} missing for a level with b != 0")
                keep.append(z)
                kz[i] = None if z is None else z.data_ptr()
        else:                                    # the entry has ONE seed: step noise on streams i + 1, known-frame noise on 0x80000000 + i
            if nz is None and solver != SOLVER_DPMPP and int(seed) != int(known.seed):
                raise _lib.DawnHipError(f"{who}: known.seed must equal the step-noise seed (the C entry takes one seed for both)")
            seed = known.seed
        return (lat.data_ptr(), msk.data_ptr(), ab, kz), seed, keep

    def _run(self, who: str, clip: dict, x_init: Tensor, steps: Sequence[dict], seed: int, noises, want_thresholds: bool,
             shard: Optional[ShardCallbacks], null_clip: Optional[dict], cond_scale: float, x0_clip, known, known_entry: bool):
        """One sampler call of any method: marshal the steps and the noises, choose the entry (_entry), then allocate, check, size the
        workspace, wire the shard, call, and raise what the call or a shard callback refused."""
        solver, step_type, kind = _SOLVERS[who]
        F, h, w = clip["F"], clip["h"], clip["w"]
        S, n, guided = len(steps), 3 * F * h * w, cond_scale != 1.0
        arr = (step_type * max(S, 1))()
        for i, st in enumerate(steps):
            for field, ctype in step_type._fields_:      # (the mirror's field names are the keys of the step dicts)
                setattr(arr[i], field, int(st[field]) if ctype is C.c_int else st[field])
        nz = None if noises is None else self._noise_ptrs(who, kind, steps, noises, n)
        name = self._entry(solver, known is not None or known_entry, x0_clip is not None, guided, shard is not None)
        known_args, keep = (), None
        if name == "dawn_sampler_run_known":
            known_args, seed, keep = self._sample_known(who, solver, known, S, F, n, seed, nz)
        x_init = x_init.contiguous().float()
        out = torch.empty_like(x_init)
        thr = torch.empty(S, 2, device=self.device) if want_thresholds else None
        if guided and null_clip is None:
            raise _lib.DawnHipError(f"{who}: cond_scale != 1 needs null_clip (prepare_null_clip)")
        mode = None if x0_clip is None else _clip_struct(x0_clip, solver == SOLVER_ANCESTRAL)
        ws = self.workspace(F, h, w, shard, guided=guided)
        comm = None
        if shard is not None:
            shard.ws = ws
            comm = C.addressof(shard.c)
        # the entries' argument lists differ in what they leave out
        args = [self.h, F, h, w, clip["mem"].data_ptr()]
        if name not in ("dawn_sampler_run", "dawn_sampler_run_sharded"):
            args += [null_clip["mem"].data_ptr() if guided else None, float(cond_scale)]
        args += [x_init.data_ptr(), S] + ([solver] if name == "dawn_sampler_run_known" else []) + [arr]
        if name != "dawn_sampler_run_dpmpp":
            args += [int(seed), nz]
        args += [out.data_ptr(), None if thr is None else thr.data_ptr(), ws.data_ptr(), ws.numel()]
        if name != "dawn_sampler_run":
            args.append(comm)
        if name not in _NO_CLIP_MODE:
            args.append(None if mode is None else C.addressof(mode))
        rc = getattr(self.L, name)(*args, *known_args, self._stream())
        del keep
        if shard is not None:
            self._shard_call(shard, rc, name)
        else:
            check(rc, name)
        return (out, thr) if want_thresholds else out

    def profile_read(self):
        """[(kind, algorithmic flops, algorithmic bytes, ms)] of the conv launches recorded under OPT_PROFILE."""
        buf = (C.c_double * (4 * 65536))()
        torch.cuda.synchronize(self.device)
        n = int(self.L.dawn_ctx_profile_read(self.h, buf, 65536))
        n = min(n, 65536)
        return [(int(buf[4 * i]), buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# C-side flow decoder (include/dawn_hip.h: dawn_decoder_* / dawn_decode_clip; csrc/dawn_decoder.hip)
class DecoderCfg(C.Structure):
    """Mirror of ``dawn_decoder_cfg``."""
    _fields_ = [("n_down", C.c_int), ("n_bottleneck", C.c_int), ("widths", C.c_int * 8)]


def decoder_named_weights(dec) -> Dict[str, Tensor]:
    """flow_decoder.FlowDecoder -> {name: device tensor} in the naming scheme of include/dawn_hip.h (decoder section)."""
    out: Dict[str, Tensor] = {"first_w3": dec.first_w3, "first_bias": dec.first_bias, "first.a": dec.first_ab[0],
                              "first.b": dec.first_ab[1], "final_w7": dec.final_w7, "final_bias": dec.final_bias}

    def conv(p: str, c):
        out[p + "w"], out[p + "bias"] = c.w, c.bias
        if c.ws is not None:
            out[p + "ws"] = c.ws
        if c.a is not None:
            out[p + "a"], out[p + "b"] = c.a, c.b

    for i, c in enumerate(dec.downs):
        conv(f"downs.{i}.", c)
    for i, c in enumerate(dec.ups):
        conv(f"ups.{i}.", c)
    for i, (ab1, c1, ab2, c2) in enumerate(dec.bott):
        out[f"bott.{i}.a1"], out[f"bott.{i}.b1"], out[f"bott.{i}.a2"], out[f"bott.{i}.b2"] = ab1[0], ab1[1], ab2[0], ab2[1]
        conv(f"bott.{i}.c1.", c1)
        conv(f"bott.{i}.c2.", c2)
    return out


class DecoderEvaluator(_Evaluator):
    """One `dawn_decoder` for one `FlowDecoder` on one device: what a non-Python host would call to turn the sampler's latent into
    frames.  PyTorch provides the device memory (packed weights, skip memory, workspace, outputs) and the stream.  `weights` lets a
    test hand in an edited table (a missing name must be an error)."""

    def __init__(self, dec, weights: Optional[Dict[str, Tensor]] = None):
        cfg = DecoderCfg()
        cfg.n_down, cfg.n_bottleneck = len(dec.downs), len(dec.bott)
        cfg.widths[0] = dec.C0
        for i, c in enumerate(dec.downs):
            cfg.widths[i + 1] = c.N
        super().__init__("dawn_decoder_create", "dawn_decoder_destroy", cfg, decoder_named_weights(dec) if weights is None else dict(weights),
                         dec.first_w3.device, fp32_only=False)

    def workspace_bytes(self, H: int, W: int, chunk: int) -> int:
        return int(self.L.dawn_decoder_workspace_bytes(self.h, H, W, chunk))

    def workspace(self, H: int, W: int, chunk: int) -> Tensor:
        return self._grown(self.workspace_bytes(H, W, chunk))

    def encode(self, img: Tensor, want_fea: bool = False):
        """img (3,H,W) fp32 contiguous -> (skip memory, fea (Cb,H/k,W/k) or None)."""
        _, H, W = img.shape
        if not (img.is_cuda and img.is_contiguous() and img.dtype == torch.float32 and img.shape[0] == 3):
            raise _lib.DawnHipError("DecoderEvaluator.encode: img must be a contiguous fp32 GPU tensor (3,H,W)")
        nb = int(self.L.dawn_decoder_skip_bytes(self.h, H, W))
        if nb == 0:
            raise _lib.DawnHipError(f"dawn_decoder_skip_bytes: {self.L.dawn_last_error().decode()}")
        mem = torch.empty(nb, dtype=torch.uint8, device=self.device)
        k = 1 << self.cfg.n_down
        fea = torch.empty(self.cfg.widths[self.cfg.n_down], H // k, W // k, device=self.device) if want_fea else None
        ws = self.workspace(H, W, 1)
        check(self.L.dawn_decoder_encode(self.h, H, W, img.data_ptr(), mem.data_ptr(), nb, None if fea is None else fea.data_ptr(),
                                         ws.data_ptr(), ws.numel(), self._stream()), "dawn_decoder_encode")
        return mem, fea

    def decode(self, img: Tensor, skip_mem: Tensor, *, T: int, h: int, w: int, chunk: int, latent: Optional[Tensor] = None,
               grid: Optional[Tensor] = None, conf: Optional[Tensor] = None, out_vid: Optional[Tensor] = None,
               warped_vid: Optional[Tensor] = None, frames: Optional[Tensor] = None, mean=(0.0, 0.0, 0.0), bgr: bool = False,
               workspace: Optional[Tensor] = None, yuv: Optional[Tensor] = None) -> None:
        """One clip: `latent` (3,T,h,w) as the sampler returns it, or `grid` (2,T,h,w) + `conf` (T,h,w).  Planes may be strided (a
        frame range of a longer clip); rows and frames must be dense.  out_vid / warped_vid: (3,T,H,W) views with dense frames;
        frames: (T,H,W,3) uint8 contiguous.  yuv: (T, 3HW/2) uint8 contiguous, the I420 frames of dawn_decode_clip_yuv420 -- the only
        output of its call (no fp32 clip, no RGB bytes, no bgr)."""
        _, H, W = img.shape
        g = latent if latent is not None else grid
        if not (g is not None and g.is_cuda and g.dtype == torch.float32 and tuple(g.shape[1:]) == (T, h, w)
                and g.stride(3) == 1 and g.stride(2) == w and g.stride(1) == h * w and g.shape[0] == (3 if latent is not None else 2)):
            raise _lib.DawnHipError("DecoderEvaluator.decode: latent (3,T,h,w) / grid (2,T,h,w) must be fp32 GPU planes with dense frames")
        if latent is None and not (conf is not None and conf.is_cuda and conf.is_contiguous() and tuple(conf.shape) == (T, h, w)
                                   and conf.dtype == torch.float32):
            raise _lib.DawnHipError("DecoderEvaluator.decode: conf must be a contiguous fp32 GPU tensor (T,h,w)")
        plane = 0
        for o in (out_vid, warped_vid):
            if o is not None:
                if not (o.is_cuda and o.dtype == torch.float32 and tuple(o.shape) == (3, T, H, W) and o.stride(3) == 1
                        and o.stride(2) == W and o.stride(1) == H * W):
                    raise _lib.DawnHipError("DecoderEvaluator.decode: out_vid / warped_vid must be fp32 (3,T,H,W) with dense frames")
                plane = o.stride(0)
        if out_vid is not None and warped_vid is not None and out_vid.stride(0) != warped_vid.stride(0):
            raise _lib.DawnHipError("DecoderEvaluator.decode: out_vid and warped_vid must share their plane stride")
        if frames is not None and not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
                                       and tuple(frames.shape) == (T, H, W, 3)):
            raise _lib.DawnHipError("DecoderEvaluator.decode: frames must be a contiguous uint8 GPU tensor (T,H,W,3)")
        ws = workspace if workspace is not None else self.workspace(H, W, max(1, min(chunk, T)))
        m = (C.c_double * 3)(*[float(v) / 255.0 for v in mean])
        p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        if yuv is not None:
            if out_vid is not None or warped_vid is not None or frames is not None or bgr:
                raise _lib.DawnHipError("DecoderEvaluator.decode: yuv is the only output of its call (no out_vid / warped_vid / frames / bgr)")
            if not (yuv.is_cuda and yuv.dtype == torch.uint8 and yuv.is_contiguous() and tuple(yuv.shape) == (T, H * W * 3 // 2)):
                raise _lib.DawnHipError("DecoderEvaluator.decode: yuv must be a contiguous uint8 GPU tensor (T, 3*H*W/2)")
            tail = (chunk, yuv.data_ptr(), m, ws.data_ptr(), ws.numel(), self._stream())
            if latent is not None:
                check(self.L.dawn_decode_clip_yuv420(self.h, H, W, T, h, w, img.data_ptr(), skip_mem.data_ptr(), latent.data_ptr(),
                                                     latent.stride(0), *tail), "dawn_decode_clip_yuv420")
            else:
                check(self.L.dawn_decode_clip_conf_yuv420(self.h, H, W, T, h, w, img.data_ptr(), skip_mem.data_ptr(), grid.data_ptr(),
                                                          grid.stride(0), conf.data_ptr(), *tail), "dawn_decode_clip_conf_yuv420")
            return
        tail = (chunk, p(out_vid), p(warped_vid), plane, p(frames), m, 1 if bgr else 0, ws.data_ptr(), ws.numel(), self._stream())
        if latent is not None:
            check(self.L.dawn_decode_clip(self.h, H, W, T, h, w, img.data_ptr(), skip_mem.data_ptr(), latent.data_ptr(),
                                          latent.stride(0), *tail), "dawn_decode_clip")
        else:
            check(self.L.dawn_decode_clip_conf(self.h, H, W, T, h, w, img.data_ptr(), skip_mem.data_ptr(), grid.data_ptr(),
                                               grid.stride(0), conf.data_ptr(), *tail), "dawn_decode_clip_conf")


# ---------------------------------------------------------------------------------------------------------------------
# C-side HuBERT audio-feature stage (include/dawn_hip.h: dawn_hubert_*; csrc/dawn_hubert.hip)
class HubertCfg(C.Structure):
    """Mirror of ``dawn_hubert_cfg``."""
    _fields_ = [("n_conv", C.c_int), ("conv_k", C.c_int * 8), ("conv_stride", C.c_int * 8), ("conv_dim", C.c_int), ("hidden", C.c_int),
                ("heads", C.c_int), ("intermediate", C.c_int), ("n_layers", C.c_int), ("pos_k", C.c_int), ("pos_groups", C.c_int),
                ("eps", C.c_float)]


def hubert_cfg(hf) -> HubertCfg:
    """hubert.HubertFeatures -> its ``dawn_hubert_cfg``."""
    if len(hf.conv) > 8 or len({c["Cout"] for c in hf.conv}) != 1:
        raise _lib.DawnHipError("dawn_hubert_cfg: at most 8 feature-extractor conv layers, all of one width")
    if len({ly["I"] for ly in hf.layers}) > 1:
        raise _lib.DawnHipError("dawn_hubert_cfg: every encoder layer must have the same intermediate width")
    cfg = HubertCfg()
    cfg.n_conv = len(hf.conv)
    for i, (c, st) in enumerate(zip(hf.conv, hf.conv_stride)):
        cfg.conv_k[i], cfg.conv_stride[i] = c["k"], st
    cfg.conv_dim, cfg.hidden, cfg.heads = hf.conv[0]["Cout"], hf.E, hf.heads
    cfg.intermediate = hf.layers[0]["I"] if hf.layers else 4
    cfg.n_layers, cfg.pos_k, cfg.pos_groups, cfg.eps = len(hf.layers), hf.pos_k, hf.pos_groups, hf.eps
    return cfg


def hubert_named_weights(hf) -> Dict[str, Tensor]:
    """hubert.HubertFeatures -> {name: device tensor} in the naming scheme of include/dawn_hip.h (HuBERT section)."""
    out: Dict[str, Tensor] = {}
    for i, c in enumerate(hf.conv):
        out[f"conv.{i}.w"], out[f"conv.{i}.g"], out[f"conv.{i}.be"] = c["w"], c["g"], c["be"]
        if c["b"] is not None:
            out[f"conv.{i}.b"] = c["b"]
    out.update({"fp.g": hf.fp_g, "fp.b": hf.fp_b, "fp.w": hf.fp_w, "fp.bias": hf.fp_bias, "pos.w": hf.pos_w_all, "pos.b": hf.pos_b,
                "enc_ln.g": hf.enc_ln[0], "enc_ln.b": hf.enc_ln[1]})
    for i, ly in enumerate(hf.layers):
        p = f"layers.{i}."
        out[p + "ln1.g"], out[p + "ln1.b"], out[p + "ln2.g"], out[p + "ln2.b"] = ly["ln1"][0], ly["ln1"][1], ly["ln2"][0], ly["ln2"][1]
        for k in ("wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2"):
            out[p + k] = ly[k]
    return out


class HubertEvaluator(_Evaluator):
    """One `dawn_hubert` for one `HubertFeatures` on one device: what a non-Python host would call to turn 16 kHz samples into the
    audio rows of `cond`.  PyTorch provides the device memory (packed weights, workspace, outputs) and the stream.  `weights` lets a
    test hand in an edited table (a missing name must be an error)."""

    MAX_SEGMENTS = 4096

    def __init__(self, hf, weights: Optional[Dict[str, Tensor]] = None):
        super().__init__("dawn_hubert_create", "dawn_hubert_destroy", hubert_cfg(hf), hubert_named_weights(hf) if weights is None else dict(weights),
                         hf.fp_w.device, fp32_only=True)

    def conv_frames(self, n: int) -> int:
        return int(self.L.dawn_hubert_conv_frames(self.h, n))

    def segments(self, n: int):
        """([(first sample, samples, rows)], expected_T, num_frames) of n samples."""
        buf, eT, nf = (C.c_long * (3 * self.MAX_SEGMENTS))(), C.c_long(0), C.c_long(0)
        ns = int(self.L.dawn_hubert_segments(self.h, n, buf, self.MAX_SEGMENTS, C.byref(eT), C.byref(nf)))
        if ns < 0:
            check(ns, "dawn_hubert_segments")
        return [tuple(buf[3 * i:3 * i + 3]) for i in range(ns)], int(eT.value), int(nf.value)

    def workspace_bytes(self, n: int) -> int:
        return int(self.L.dawn_hubert_workspace_bytes(self.h, n))

    def workspace(self, n: int) -> Tensor:
        return self._grown(self.workspace_bytes(n))

    def _samples(self, x: Tensor, who: str) -> None:
        if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 1):
            raise _lib.DawnHipError(f"HubertEvaluator.{who}: samples must be a contiguous 1-D fp32 GPU tensor")

    def encode(self, x: Tensor, workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        """x (n,) normalised samples of one segment -> last_hidden_state (T', E)."""
        self._samples(x, "encode")
        n = x.numel()
        ws = workspace if workspace is not None else self.workspace(n)
        if out is None:
            out = torch.empty(self.conv_frames(n), self.cfg.hidden, device=self.device)
        check(self.L.dawn_hubert_encode(self.h, x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
              "dawn_hubert_encode")
        return out

    def features(self, speech: Tensor, workspace: Optional[Tensor] = None, hidden: Optional[Tensor] = None,
                 target: Optional[Tensor] = None, want_hidden: bool = True):
        """speech (n,) raw fp32 samples -> (hidden (expected_T, E) or None, target (num_frames, E)): all of process_audio."""
        self._samples(speech, "features")
        n = speech.numel()
        _, eT, nf = self.segments(n)
        ws = workspace if workspace is not None else self.workspace(n)
        if hidden is None and want_hidden:
            hidden = torch.empty(eT, self.cfg.hidden, device=self.device)
        if target is None:
            target = torch.empty(nf, self.cfg.hidden, device=self.device)
        check(self.L.dawn_hubert_features(self.h, speech.data_ptr(), n, None if hidden is None else hidden.data_ptr(), target.data_ptr(),
                                          ws.data_ptr(), ws.numel(), self._stream()), "dawn_hubert_features")
        return hidden, target


# ---------------------------------------------------------------------------------------------------------------------
# C-side PBnet pose / blink stage (include/dawn_hip.h: dawn_pbnet_*, dawn_pose_blink_stage; csrc/dawn_pbnet.hip)
class PbnetCfg(C.Structure):
    """Mirror of ``dawn_pbnet_cfg``."""
    _fields_ = [("in_dim", C.c_int), ("audio_dim", C.c_int), ("latent_dim", C.c_int), ("d", C.c_int), ("heads", C.c_int), ("ff", C.c_int),
                ("n_layers", C.c_int), ("win", C.c_int), ("nrot", C.c_int), ("eps", C.c_float)]


_PB_FREQS = "init_temporal_attn.fn.fn.rotary_emb.freqs"


def pbnet_cfg(gen) -> PbnetCfg:
    """pbnet.PoseBlinkGenerator -> its ``dawn_pbnet_cfg``."""
    w = gen.w
    if w["audioEmbedding.weight"].shape[0] != gen.latent_dim:
        raise _lib.DawnHipError("dawn_pbnet_cfg: 'audioEmbedding.weight' must be as wide as the latent (ztimelinear reads d + 2 * latent_dim)")
    ffs = {w[f"seqTransDecoder.decoder_layers.{i}.ffn.linear1.weight"].shape[0] for i in range(gen.n_layers)}
    if len(ffs) > 1:
        raise _lib.DawnHipError("dawn_pbnet_cfg: every decoder layer must have the same FFN width")
    cfg = PbnetCfg()
    cfg.in_dim, cfg.audio_dim, cfg.latent_dim, cfg.d, cfg.heads = gen.in_dim, gen.audio_dim, gen.latent_dim, gen.d, gen.heads
    cfg.ff, cfg.n_layers, cfg.win, cfg.nrot, cfg.eps = (ffs.pop() if ffs else 4), gen.n_layers, gen.window, w[_PB_FREQS].numel(), 1e-5
    return cfg


def pbnet_named_weights(gen) -> Dict[str, Tensor]:
    """pbnet.PoseBlinkGenerator -> {name: device tensor} in the naming scheme of include/dawn_hip.h (PBnet section): the decoder's own
    state_dict keys plus the three tables built here -- the two O(window) bias tables and every layer's [to_k ; to_v] in one image.
    Only pointers reach the C side, so the shapes it relies on are checked here, by name."""
    w, d, hd, dev = gen.w, gen.d, gen.heads * 32, gen.device
    layers = [f"seqTransDecoder.decoder_layers.{i}." for i in range(gen.n_layers)]
    ff = w[layers[0] + "ffn.linear1.weight"].shape[0] if layers else 4
    want = {"firstposeEmbedding.weight": (d, gen.in_dim), "firstposeEmbedding.bias": (d,),
            "audioEmbedding.weight": (gen.latent_dim, gen.audio_dim), "audioEmbedding.bias": (gen.latent_dim,),
            "ztimelinear.weight": (d, d + 2 * gen.latent_dim), "ztimelinear.bias": (d,), "init_proj.bias": (d,),
            "init_temporal_attn.fn.norm.gamma": (d,), "init_temporal_attn.fn.norm.beta": (d,),
            "init_temporal_attn.fn.fn.to_qkv.weight": (3 * hd, d), "init_temporal_attn.fn.fn.to_out.weight": (d, hd),
            _PB_FREQS: (w[_PB_FREQS].numel(),), "finallayer.weight": (gen.in_dim, d), "finallayer.bias": (gen.in_dim,)}
    for p in layers:
        want.update({p + "self_attn.to_qkv.weight": (3 * hd, d), p + "self_attn.to_out.weight": (d, hd),
                     p + "multihead_attn.to_q.weight": (hd, d), p + "multihead_attn.to_out.weight": (d, hd),
                     p + "ffn.linear1.weight": (ff, d), p + "ffn.linear1.bias": (ff,), p + "ffn.linear2.weight": (d, ff),
                     p + "ffn.linear2.bias": (d,)})
        for n in (1, 2, 3):
            want.update({p + f"layer_norm{n}.weight": (d,), p + f"layer_norm{n}.bias": (d,)})
    out: Dict[str, Tensor] = {}
    for k, shape in want.items():
        if k not in w:
            raise _lib.DawnHipError(f"pbnet_named_weights: the decoder lacks '{k}'")
        if tuple(w[k].shape) != shape:
            raise _lib.DawnHipError(f"pbnet_named_weights: '{k}' is {tuple(w[k].shape)}, {shape} expected (heads of 32, d = {d})")
        out[k] = w[k]
    kv = []
    for p in layers:
        for n in ("multihead_attn.to_k.weight", "multihead_attn.to_v.weight"):
            if p + n not in w or tuple(w[p + n].shape) != (hd, d):
                raise _lib.DawnHipError(f"pbnet_named_weights: '{p + n}' missing or not {(hd, d)}")
            kv.append(w[p + n])
    if kv:
        out["mem_kv.w"] = torch.cat(kv, 0).contiguous()
    out["bias_tgt.rel"] = gen.rel_bias("tgt").to(dev)
    out["bias_mem.rel"] = gen.rel_bias("mem").to(dev)
    return out


class PbnetEvaluator(_Evaluator):
    """One `dawn_pbnet` for one `PoseBlinkGenerator` on one device: what a non-Python host would call to produce the pose or blink
    columns of `cond`.  PyTorch provides the device memory (weights, workspace, outputs) and the stream.  `weights` lets a test hand in
    an edited table (a missing name must be an error)."""

    def __init__(self, gen, weights: Optional[Dict[str, Tensor]] = None):
        super().__init__("dawn_pbnet_create", "dawn_pbnet_destroy", pbnet_cfg(gen), pbnet_named_weights(gen) if weights is None else dict(weights),
                         gen.device, fp32_only=True)

    def workspace_bytes(self, T: int) -> int:
        return int(self.L.dawn_pbnet_workspace_bytes(self.h, T))

    def workspace(self, T: int) -> Tensor:
        return self._grown(self.workspace_bytes(T))

    def generate(self, x0: Tensor, audio: Tensor, z: Tensor, workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        """x0 (in_dim) first pose, audio (T, audio_dim) (rows may be strided), z (T, latent_dim) -> (T, in_dim): `_decode_one`.
        `out`: a (T, in_dim) view with unit column stride (a column slice of a wider buffer is fine)."""
        T = audio.shape[0]
        for t, shape, name in ((x0, (self.cfg.in_dim,), "x0"), (audio, (T, self.cfg.audio_dim), "audio"), (z, (T, self.cfg.latent_dim), "z")):
            if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == shape and t.stride(-1) == 1):
                raise _lib.DawnHipError(f"PbnetEvaluator.generate: {name} must be an fp32 GPU tensor of shape {shape}")
        if not z.is_contiguous():
            raise _lib.DawnHipError("PbnetEvaluator.generate: z must be contiguous")
        ws = workspace if workspace is not None else self.workspace(T)
        if out is None:
            out = torch.empty(T, self.cfg.in_dim, device=self.device)
        if not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (T, self.cfg.in_dim) and out.stride(1) == 1):
            raise _lib.DawnHipError("PbnetEvaluator.generate: out must be an fp32 GPU (T, in_dim) view with unit column stride")
        check(self.L.dawn_pbnet_generate(self.h, x0.data_ptr(), audio.data_ptr(), audio.stride(0) if T > 1 else self.cfg.audio_dim,
                                         z.data_ptr(), T, out.data_ptr(), out.stride(0) if T > 1 else self.cfg.in_dim, ws.data_ptr(),
                                         ws.numel(), self._stream()), "dawn_pbnet_generate")
        return out


def pose_blink_stage_c(ev_pose: PbnetEvaluator, ev_blink: PbnetEvaluator, audio: Tensor, init_pose6, init_blink2, z_pose: Tensor,
                       z_blink: Tensor, dri_pose: Optional[Tensor] = None, dri_blink: Optional[Tensor] = None,
                       workspace: Optional[Tensor] = None):
    """dawn_pose_blink_stage: audio (T, audio_dim) and the latents (T, latent_dim) on the device, the two initial rows as host numbers
    -> (dri_pose (T, 6), dri_blink (T, 2)) on the device; `dri_pose` / `dri_blink` may be column slices of wider buffers."""
    L, T = ev_pose.L, audio.shape[0]
    for t, w, name in ((audio, ev_pose.cfg.audio_dim, "audio"), (z_pose, ev_pose.cfg.latent_dim, "z_pose"),
                       (z_blink, ev_blink.cfg.latent_dim, "z_blink")):
        if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (T, w) and t.stride(1) == 1) or \
                (name != "audio" and not t.is_contiguous()):
            raise _lib.DawnHipError(f"pose_blink_stage_c: {name} must be an fp32 GPU tensor of shape {(T, w)}")
    ip = (C.c_float * 6)(*[float(v) for v in init_pose6])
    ib = (C.c_float * 2)(*[float(v) for v in init_blink2])
    if dri_pose is None:
        dri_pose = torch.empty(T, 6, device=audio.device)
    if dri_blink is None:
        dri_blink = torch.empty(T, 2, device=audio.device)
    for t, w in ((dri_pose, 6), (dri_blink, 2)):
        if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (T, w) and t.stride(1) == 1):
            raise _lib.DawnHipError(f"pose_blink_stage_c: outputs must be fp32 GPU (T, {w}) views with unit column stride")
    need = int(L.dawn_pose_blink_workspace_bytes(ev_pose.h, ev_blink.h, T))
    ws = workspace if workspace is not None else ev_pose._grown(need)
    ld = lambda t, w: t.stride(0) if T > 1 else w                                             # noqa: E731
    check(L.dawn_pose_blink_stage(ev_pose.h, ev_blink.h, audio.data_ptr(), ld(audio, ev_pose.cfg.audio_dim), T, ip, ib, z_pose.data_ptr(),
                                  z_blink.data_ptr(), dri_pose.data_ptr(), ld(dri_pose, 6), dri_blink.data_ptr(), ld(dri_blink, 2),
                                  ws.data_ptr(), ws.numel(), ev_pose._stream()), "dawn_pose_blink_stage")
    return dri_pose, dri_blink


# ---------------------------------------------------------------------------------------------------------------------
# C-side clip-input stage (include/dawn_hip.h: dawn_inputs_*, dawn_clip_inputs; csrc/dawn_inputs.hip)
class InputsCfg(C.Structure):
    """Mirror of ``dawn_inputs_cfg``."""
    _fields_ = [("n_aud", C.c_int), ("pose_dim", C.c_int), ("eye_dim", C.c_int)]


_FACE_LOC = {"face_loc_emb.conv1.weight": (8, 1, 3, 3), "face_loc_emb.conv1.bias": (8,), "face_loc_emb.conv2.weight": (16, 8, 3, 3),
             "face_loc_emb.conv2.bias": (16,)}


def inputs_named_weights(flow_diffusion) -> Dict[str, Tensor]:
    """flow_diffusion.FlowDiffusion -> {state_dict key: device tensor} of its Face_loc_Encoder (the reference never saves it:
    whatever the module holds).  Only pointers reach the C side, so the shapes are checked here."""
    sd = flow_diffusion.state_dict()
    out: Dict[str, Tensor] = {}
    for k, shape in _FACE_LOC.items():
        if k not in sd or tuple(sd[k].shape) != shape:
            raise _lib.DawnHipError(f"inputs_named_weights: '{k}' missing or not {shape}")
        out[k] = sd[k].detach()
    return out


def _host_floats(v, n: Optional[int] = None):
    if v is None:
        return None
    v = [float(x) for x in v]
    if n is not None and len(v) != n:
        raise _lib.DawnHipError(f"{n} host numbers expected, {len(v)} given")
    return (C.c_float * len(v))(*v)


class InputsEvaluator(_Evaluator):
    """One `dawn_inputs` for one `FlowDiffusion` on one device: what a non-Python host would call for the face-location channels of
    fea272 and the condition rows.  PyTorch provides the device memory and the stream.  `weights` lets a test hand in an edited table."""

    def __init__(self, flow_diffusion, n_aud: int = 1024, weights: Optional[Dict[str, Tensor]] = None, pose_dim: Optional[int] = None):
        cfg = InputsCfg(int(n_aud), int(flow_diffusion.pose_dim if pose_dim is None else pose_dim), 2)
        w = inputs_named_weights(flow_diffusion) if weights is None else dict(weights)
        dev = next(iter(w.values())).device if w else torch.device("cuda")
        super().__init__("dawn_inputs_create", "dawn_inputs_destroy", cfg, w, dev, fp32_only=True)

    def clip_inputs(self, bbox6, size: int, fea: Tensor, audio: Tensor, pose: Tensor, eye: Tensor, init_pose=None, init_eye=None,
                    cond: Optional[Tensor] = None) -> Tensor:
        """dawn_clip_inputs: `fea` = fea272 (fea_ch, size/4, size/4) contiguous -- or just its last 16 planes --, whose last 16 planes are
        written; audio (T, n_aud), pose (T, n_pose), eye (T, 2) rows with unit column stride (they may be the column views of `cond`
        they land in); init_pose / init_eye host numbers or None -> cond (T, n_aud + pose_dim + 2) (allocated when None)."""
        T, P = audio.shape[0], self.cfg.pose_dim
        width = self.cfg.n_aud + P + 2
        if cond is None:
            cond = torch.empty(T, width, device=self.device)
        for t, w_, name in ((audio, self.cfg.n_aud, "audio"), (pose, pose.shape[1], "pose"), (eye, 2, "eye"), (cond, cond.shape[1], "cond")):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (T, w_) and t.stride(1) == 1):
                raise _lib.DawnHipError(f"InputsEvaluator.clip_inputs: {name} must be an fp32 GPU tensor of shape {(T, w_)} with unit column stride")
        if not (fea.is_cuda and fea.dtype == torch.float32 and fea.is_contiguous() and fea.dim() == 3 and fea.shape[0] >= 16
                and tuple(fea.shape[1:]) == (size // 4, size // 4)):
            raise _lib.DawnHipError("InputsEvaluator.clip_inputs: fea must be a contiguous fp32 GPU tensor (>= 16, size/4, size/4)")
        ld = lambda t: t.stride(0) if T > 1 else max(t.stride(0), t.shape[1])                    # noqa: E731
        ip = _host_floats(init_pose)
        check(self.L.dawn_clip_inputs(self.h, _host_floats(bbox6, 6), int(size), fea.data_ptr(), fea.shape[0], audio.data_ptr(), ld(audio),
                                      pose.data_ptr(), pose.shape[1], ld(pose), eye.data_ptr(), ld(eye), ip, 0 if ip is None else len(ip),
                                      _host_floats(init_eye, 2), T, cond.data_ptr(), ld(cond), self._stream()), "dawn_clip_inputs")
        return cond


# ---------------------------------------------------------------------------------------------------------------------
# one call from samples and a source image to frame bytes (include/dawn_hip.h: dawn_generate_bytes / dawn_generate_clip)
class GenerateArgs(C.Structure):
    """Mirror of ``dawn_generate_args``."""
    _fields_ = [("hubert", C.c_void_p), ("pose", C.c_void_p), ("blink", C.c_void_p), ("decoder", C.c_void_p), ("inputs", C.c_void_p),
                ("unet", C.c_void_p), ("samples", C.c_void_p), ("n_samples", C.c_long), ("img3", C.c_void_p), ("H", C.c_int),
                ("fea_ch", C.c_int), ("bbox6", C.POINTER(C.c_float)), ("init_pose", C.POINTER(C.c_float)),
                ("init_eye", C.POINTER(C.c_float)), ("n_init", C.c_int), ("latent_dim", C.c_int), ("init_pose6", C.POINTER(C.c_float)),
                ("init_blink2", C.POINTER(C.c_float)), ("T", C.c_long), ("S", C.c_int), ("cond_scale", C.c_float),
                ("ddim_steps", C.POINTER(DdimStep)), ("ancestral_steps", C.POINTER(AncestralStep)), ("clip", C.POINTER(ClipMode)),
                ("seed", C.c_uint64), ("format", C.c_int), ("bgr", C.c_int), ("chunk", C.c_int), ("mean3", C.POINTER(C.c_double)),
                ("frames_out", C.c_void_p), ("latent_out", C.c_void_p), ("cond_out", C.c_void_p)]


class MediaArgs(C.Structure):
    """Mirror of ``dawn_media_args``."""
    _fields_ = [("gen", C.POINTER(GenerateArgs)), ("image", C.c_void_p), ("Hs", C.c_int), ("Ws", C.c_int), ("row_bytes", C.c_long),
                ("pix_bytes", C.c_int), ("order", C.c_int), ("pcm", C.c_void_p), ("n_frames", C.c_long), ("channels", C.c_int)]


FRAMES_RGB, FRAMES_YUV420 = 0, 1
PIXELS_RGB, PIXELS_BGR = 0, 1
Z_POSE_STREAM, Z_BLINK_STREAM = 0xFFFFFFFE, 0xFFFFFFFF      # Philox stream ids of the PBnet latents; x_init is stream 0, sampler steps 1..


class PipelineEvaluator:
    """dawn_generate_clip over the five stage evaluators (they own the handles and keep the weights alive): samples + image -> frame
    bytes in one C call.  PyTorch provides the device memory (inputs, outputs, one grow-only workspace) and the stream."""

    def __init__(self, hubert: HubertEvaluator, pose: PbnetEvaluator, blink: PbnetEvaluator, decoder: DecoderEvaluator,
                 inputs: InputsEvaluator, unet: CtxEvaluator):
        self.L = _lib.lib()
        self.ev = (hubert, pose, blink, decoder, inputs, unet)
        self.device = unet.device
        self._ws: Optional[Tensor] = None

    def args(self, samples: Tensor, img: Tensor, bbox6, init_pose6, init_blink2, T: int, steps: Sequence[dict], *, ancestral: bool = False,
             init_pose=None, init_eye=None, cond_scale: float = 1.0, x0_clip=None, seed: int = 0, fmt: str = "rgb", mean=(0.0, 0.0, 0.0),
             bgr: bool = False, chunk: int = 16, H: Optional[int] = None) -> GenerateArgs:
        """The filled struct; every host array it points to is kept alive on it (`_keep`).  samples / img may be None where
        `from_media` supplies PCM / image bytes instead; without an img the model's image side is `H`."""
        hub, pose, blink, dec, inp, unet = self.ev
        if samples is not None and not (samples.is_cuda and samples.is_contiguous() and samples.dtype == torch.float32 and samples.dim() == 1):
            raise _lib.DawnHipError("PipelineEvaluator: samples must be a contiguous 1-D fp32 GPU tensor")
        if img is None and H is None:
            raise _lib.DawnHipError("PipelineEvaluator: without an img the image side H must be given")
        if img is not None and not (img.is_cuda and img.is_contiguous() and img.dtype == torch.float32 and img.dim() == 3 and img.shape[0] == 3
                                    and img.shape[1] == img.shape[2] and H in (None, img.shape[1])):
            raise _lib.DawnHipError("PipelineEvaluator: img must be a contiguous fp32 GPU tensor (3, H, H)")
        if fmt not in ("rgb", "yuv420p"):
            raise _lib.DawnHipError(f"PipelineEvaluator: format must be 'rgb' or 'yuv420p', not {fmt!r}")
        a = GenerateArgs()
        a.hubert, a.pose, a.blink, a.decoder, a.inputs, a.unet = hub.h, pose.h, blink.h, dec.h, inp.h, unet.h
        if samples is not None:
            a.samples, a.n_samples = samples.data_ptr(), samples.numel()
        if img is not None:
            a.img3 = img.data_ptr()
        a.H, a.fea_ch = int(H if img is None else img.shape[1]), unet.cfg.fea_ch
        S = len(steps)
        if ancestral:
            arr = (AncestralStep * max(S, 1))()
            for i, st in enumerate(steps):
                arr[i].t, arr[i].recip, arr[i].recipm1 = int(st["t"]), st["recip"], st["recipm1"]
                arr[i].c1, arr[i].c2, arr[i].std = st["c1"], st["c2"], st["std"]
            a.ancestral_steps = arr
        else:
            arr = (DdimStep * max(S, 1))()
            for i, st in enumerate(steps):
                arr[i].t, arr[i].t_next = int(st["t"]), int(st["t_next"])
                arr[i].recip, arr[i].recipm1 = st["recip"], st["recipm1"]
                arr[i].sqrt_alpha_next, arr[i].c, arr[i].sigma = st["sqrt_alpha_next"], st["c"], st["sigma"]
            a.ddim_steps = arr
        keep = [arr, _host_floats(bbox6, 6), _host_floats(init_pose), _host_floats(init_eye, 2), _host_floats(init_pose6, 6),
                _host_floats(init_blink2, 2), (C.c_double * 3)(*[float(v) / 255.0 for v in mean])]
        if keep[1] is not None:
            a.bbox6 = keep[1]
        if keep[2] is not None:
            a.init_pose, a.n_init = keep[2], len(keep[2])
        if keep[3] is not None:
            a.init_eye = keep[3]
        a.init_pose6, a.init_blink2, a.mean3 = keep[4], keep[5], keep[6]
        if x0_clip is not None:
            keep.append(_clip_struct(x0_clip, ancestral))
            a.clip = C.pointer(keep[-1])
        a.latent_dim, a.T, a.S, a.cond_scale, a.seed = pose.cfg.latent_dim, int(T), S, float(cond_scale), int(seed)
        a.format, a.bgr, a.chunk = (FRAMES_YUV420 if fmt == "yuv420p" else FRAMES_RGB), int(bool(bgr)), int(chunk)
        a._keep = keep
        return a

    def sizes(self, a: GenerateArgs):
        """(bytes of the frames, bytes of the workspace) of dawn_generate_bytes."""
        cb, wb = C.c_size_t(0), C.c_size_t(0)
        check(self.L.dawn_generate_bytes(C.addressof(a), C.byref(cb), C.byref(wb)), "dawn_generate_bytes")
        return int(cb.value), int(wb.value)

    def generate(self, a: GenerateArgs, want_latent: bool = False, want_cond: bool = False, workspace: Optional[Tensor] = None,
                 frames: Optional[Tensor] = None) -> dict:
        """Run dawn_generate_clip on the struct of `args(...)` -> {"frames": uint8 (T,H,H,3) or (T, 3HH/2), "latent", "cond"}."""
        hub, pose, blink, dec, inp, unet = self.ev
        cb, wb = self.sizes(a)
        T, H, h = int(a.T), int(a.H), int(a.H) // 4
        if frames is None:
            frames = torch.empty((T, H * H * 3 // 2) if a.format == FRAMES_YUV420 else (T, H, H, 3), dtype=torch.uint8, device=self.device)
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.numel() == cb):
            raise _lib.DawnHipError(f"PipelineEvaluator.generate: frames must be a contiguous uint8 GPU tensor of {cb} bytes")
        out = {"frames": frames}
        a.frames_out = frames.data_ptr()
        if want_latent:
            out["latent"] = torch.empty(3, T, h, h, device=self.device)
            a.latent_out = out["latent"].data_ptr()
        if want_cond:
            out["cond"] = torch.empty(T, inp.cfg.n_aud + inp.cfg.pose_dim + 2, device=self.device)
            a.cond_out = out["cond"].data_ptr()
        if want_latent or want_cond:
            cb, wb = self.sizes(a)                          # (outputs the caller takes leave the workspace)
        if workspace is None:
            if self._ws is None or self._ws.numel() < wb:
                self._ws = None
                self._ws = torch.empty(wb, dtype=torch.uint8, device=self.device)
            workspace = self._ws
        check(self.L.dawn_generate_clip(C.addressof(a), workspace.data_ptr(), workspace.numel(), _Evaluator._stream()), "dawn_generate_clip")
        return out

    # ---- the same from decoded media (dawn_generate_media_bytes / dawn_generate_clip_media)
    def from_media(self, a: GenerateArgs, image: Optional[Tensor] = None, pcm: Optional[Tensor] = None, order: str = "rgb",
                   pcm_rate: int = 16000) -> MediaArgs:
        """`a` = the struct of `args(...)` (its img / samples are placeholders for whatever is given here) -> the dawn_media_args that
        replaces them: image = uint8 GPU tensor (Hs, Ws, C) or (Hs, Ws) with unit pixel and channel strides and any row stride, C in
        {1, 3, 4}; pcm = int16 GPU tensor (n_frames, channels) or (n_frames,), contiguous.  None keeps the input of `a`.
        pcm_rate = the sample rate of `pcm` (the struct has no field for it: it is kept beside it, and `media_sizes` / `generate_media`
        hand it to the *_rate entry points; 16000 = the entry points without a rate)."""
        m = MediaArgs()
        m._pcm_rate = int(pcm_rate)
        m.gen = C.pointer(a)
        keep = [a]
        if image is not None:
            pb = 1 if image.dim() == 2 else int(image.shape[2])
            if not (image.is_cuda and image.dtype == torch.uint8 and image.dim() in (2, 3) and image.stride(1) == pb
                    and (image.dim() == 2 or image.stride(2) == 1)):
                raise _lib.DawnHipError("PipelineEvaluator.from_media: image must be a uint8 GPU tensor (Hs, Ws[, C]) with dense pixels")
            if order not in ("rgb", "bgr"):
                raise _lib.DawnHipError(f"PipelineEvaluator.from_media: order must be 'rgb' or 'bgr', not {order!r}")
            m.image, m.Hs, m.Ws, m.pix_bytes = image.data_ptr(), int(image.shape[0]), int(image.shape[1]), pb
            m.row_bytes = int(image.stride(0)) if image.shape[0] > 1 else max(int(image.stride(0)), int(image.shape[1]) * pb)
            m.order = PIXELS_BGR if order == "bgr" else PIXELS_RGB
            keep.append(image)
        if pcm is not None:
            if not (pcm.is_cuda and pcm.dtype == torch.int16 and pcm.dim() in (1, 2) and pcm.is_contiguous()):
                raise _lib.DawnHipError("PipelineEvaluator.from_media: pcm must be a contiguous int16 GPU tensor (n_frames[, channels])")
            m.pcm, m.n_frames, m.channels = pcm.data_ptr(), int(pcm.shape[0]), 1 if pcm.dim() == 1 else int(pcm.shape[1])
            keep.append(pcm)
        m._keep = keep
        return m

    @staticmethod
    def _rate_of(m: MediaArgs, pcm_rate: Optional[int]) -> int:
        return int(getattr(m, "_pcm_rate", 16000) if pcm_rate is None else pcm_rate)

    def media_sizes(self, m: MediaArgs, pcm_rate: Optional[int] = None):
        """(bytes of the frames, bytes of the workspace) of dawn_generate_media_bytes -- of dawn_generate_media_rate_bytes where the PCM is
        not at 16 kHz.  pcm_rate None: the rate `from_media` was given (16000 unless stated)."""
        cb, wb = C.c_size_t(0), C.c_size_t(0)
        rate = self._rate_of(m, pcm_rate)
        if rate == 16000:
            check(self.L.dawn_generate_media_bytes(C.addressof(m), C.byref(cb), C.byref(wb)), "dawn_generate_media_bytes")
        else:
            check(self.L.dawn_generate_media_rate_bytes(C.addressof(m), rate, C.byref(cb), C.byref(wb)), "dawn_generate_media_rate_bytes")
        return int(cb.value), int(wb.value)

    def generate_media(self, m: MediaArgs, want_latent: bool = False, want_cond: bool = False, workspace: Optional[Tensor] = None,
                       frames: Optional[Tensor] = None, pcm_rate: Optional[int] = None) -> dict:
        """`generate` through dawn_generate_clip_media on the struct of `from_media(...)`: the same outputs.  With PCM at another rate
        than 16 kHz (pcm_rate None: the rate `from_media` was given) through dawn_generate_clip_media_rate, which resamples it first."""
        hub, pose, blink, dec, inp, unet = self.ev
        a = m.gen.contents
        rate = self._rate_of(m, pcm_rate)
        cb, wb = self.media_sizes(m, rate)
        T, H, h = int(a.T), int(a.H), int(a.H) // 4
        if frames is None:
            frames = torch.empty((T, H * H * 3 // 2) if a.format == FRAMES_YUV420 else (T, H, H, 3), dtype=torch.uint8, device=self.device)
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.numel() == cb):
            raise _lib.DawnHipError(f"PipelineEvaluator.generate_media: frames must be a contiguous uint8 GPU tensor of {cb} bytes")
        out = {"frames": frames}
        a.frames_out = frames.data_ptr()
        if want_latent:
            out["latent"] = torch.empty(3, T, h, h, device=self.device)
            a.latent_out = out["latent"].data_ptr()
        if want_cond:
            out["cond"] = torch.empty(T, inp.cfg.n_aud + inp.cfg.pose_dim + 2, device=self.device)
            a.cond_out = out["cond"].data_ptr()
        if want_latent or want_cond:
            cb, wb = self.media_sizes(m, rate)
        if workspace is None:
            if self._ws is None or self._ws.numel() < wb:
                self._ws = None
                self._ws = torch.empty(wb, dtype=torch.uint8, device=self.device)
            workspace = self._ws
        if rate == 16000:
            check(self.L.dawn_generate_clip_media(C.addressof(m), workspace.data_ptr(), workspace.numel(), _Evaluator._stream()),
                  "dawn_generate_clip_media")
        else:
            check(self.L.dawn_generate_clip_media_rate(C.addressof(m), rate, workspace.data_ptr(), workspace.numel(), _Evaluator._stream()),
                  "dawn_generate_clip_media_rate")
        return out


# ---------------------------------------------------------------------------------------------------------------------
# C-side motion-encode stage (include/dawn_hip.h: dawn_motion_*, dawn_reenact_*; csrc/dawn_motion.hip)
MOTION_MAX_BLOCKS = 8


class MotionCfg(C.Structure):
    """Mirror of ``dawn_motion_cfg``."""
    _fields_ = [("R", C.c_int), ("s", C.c_int), ("temperature", C.c_double), ("rp_blocks", C.c_int), ("bg_blocks", C.c_int), ("pf_blocks", C.c_int),
                ("rp_down", C.c_int * MOTION_MAX_BLOCKS), ("rp_up", C.c_int * MOTION_MAX_BLOCKS), ("bg_down", C.c_int * MOTION_MAX_BLOCKS),
                ("pf_down", C.c_int * MOTION_MAX_BLOCKS), ("pf_up", C.c_int * MOTION_MAX_BLOCKS)]


class ReenactArgs(C.Structure):
    """Mirror of ``dawn_reenact_args``."""
    _fields_ = [("size", C.c_size_t), ("motion", C.c_void_p), ("decoder", C.c_void_p), ("img3", C.c_void_p), ("H", C.c_int), ("W", C.c_int),
                ("drv", C.c_void_p), ("drv_kind", C.c_int), ("T", C.c_int), ("drv_frame_stride", C.c_long), ("drv_chan_stride", C.c_long),
                ("motion_chunk", C.c_int), ("chunk", C.c_int), ("format", C.c_int), ("bgr", C.c_int), ("mean3", C.POINTER(C.c_double)),
                ("frames_out", C.c_void_p), ("grid_out", C.c_void_p), ("conf_out", C.c_void_p)]


def motion_cfg(enc) -> MotionCfg:
    """motion_encoder.MotionEncoder -> its ``dawn_motion_cfg``: R, s, temperature and the REAL channel counts of the three conv stacks
    (the packed images hold each rounded up to a multiple of 16; motion_encoder.pad16 is the one definition of that)."""
    stacks = (("rp_down", enc.rp_hg.enc.reals), ("rp_up", enc.rp_hg.up_reals), ("bg_down", enc.bg_enc.reals),
              ("pf_down", enc.pf_hg.enc.reals), ("pf_up", enc.pf_hg.up_reals))
    cfg = MotionCfg()
    cfg.R, cfg.s, cfg.temperature = enc.R, enc.s, enc.temperature
    cfg.rp_blocks, cfg.bg_blocks, cfg.pf_blocks = enc.rp_hg.levels, len(enc.bg_enc.downs), enc.pf_hg.levels
    for name, reals in stacks:
        if not 1 <= len(reals) <= MOTION_MAX_BLOCKS:
            raise _lib.DawnHipError(f"dawn_motion_cfg: {name} has {len(reals)} blocks, 1 .. {MOTION_MAX_BLOCKS} fit the struct")
        arr = getattr(cfg, name)
        for i, c in enumerate(reals):
            arr[i] = int(c)
    return cfg


def motion_named_weights(enc) -> Dict[str, Tensor]:
    """motion_encoder.MotionEncoder -> {name: device tensor} in the naming scheme of include/dawn_hip.h (motion stage): the packed _Conv
    images as they are.  The background encoder's first conv travels as its two halves (bg.src0 with the bias, bg.drv0), its BatchNorm
    as bg.down.0.a / b; the unsplit 6-channel image of that conv is not in the table (nothing launches it)."""
    out: Dict[str, Tensor] = {}

    def conv(p: str, c, norm: bool = True):
        out[p + "w"] = c.w
        if c.ws is not None:
            out[p + "ws"] = c.ws
        if c.bias is not None:
            out[p + "bias"] = c.bias
        if norm and c.a is not None:
            out[p + "a"], out[p + "b"] = c.a, c.b

    for stem, hg in (("rp.", enc.rp_hg), ("pf.", enc.pf_hg)):
        for i, c in enumerate(hg.enc.downs):
            conv(f"{stem}down.{i}.", c)
        for i, c in enumerate(hg.ups):
            conv(f"{stem}up.{i}.", c)
    conv("rp.regions.", enc.rp_regions)
    conv("pf.out.", enc.pf_out)
    conv("bg.src0.", enc.bg_src0)
    conv("bg.drv0.", enc.bg_drv0, norm=False)
    out["bg.down.0.a"], out["bg.down.0.b"] = enc.bg_enc.downs[0].a, enc.bg_enc.downs[0].b
    for i, c in enumerate(enc.bg_enc.downs[1:], 1):
        conv(f"bg.down.{i}.", c)
    out["fc.w"], out["fc.b"] = enc.fc_w, enc.fc_b
    return out


class MotionEvaluator(_Evaluator):
    """One `dawn_motion` on one device: what a non-Python host would call to turn a driving video into the flow / occlusion latent.
    Built from a `MotionEncoder` (its packed weights, kept alive here) -- or, `handle=`, around a handle that a bundle made
    (BundleEvaluator.motion(): the bundle owns the weights).  PyTorch provides the device memory and the stream."""

    def __init__(self, enc=None, weights: Optional[Dict[str, Tensor]] = None, *, handle=None, cfg: Optional[MotionCfg] = None, device=None,
                 keep=None):
        if handle is not None:
            self.L = _lib.lib()
            self.device, self.cfg, self.weights, self._destroy, self.h, self._ws, self._keep = torch.device(device), cfg, {}, "dawn_motion_destroy", handle, None, keep
            return
        super().__init__("dawn_motion_create", "dawn_motion_destroy", motion_cfg(enc), motion_named_weights(enc) if weights is None else dict(weights),
                         enc.device, fp32_only=False)

    def latent_size(self, H: int, W: int) -> Tuple[int, int]:
        s = self.cfg.s
        return -(-H // s), -(-W // s)

    def workspace_bytes(self, H: int, W: int, chunk: int) -> int:
        return int(self.L.dawn_motion_workspace_bytes(self.h, H, W, chunk))

    def workspace(self, H: int, W: int, chunk: int) -> Tensor:
        return self._grown(self.workspace_bytes(H, W, chunk))

    @staticmethod
    def _source(src: Tensor):
        """-> (tensor kept alive, kind, H, W) of a source image: fp32 (3,H,W) / (1,3,H,W), or uint8 (1,H,W,3)."""
        if src.dtype == torch.uint8:
            if src.dim() != 4 or src.shape[0] != 1 or src.shape[3] != 3:
                raise _lib.DawnHipError("MotionEvaluator: a uint8 source image is (1,H,W,3)")
            return src.contiguous(), 1, int(src.shape[1]), int(src.shape[2])
        src = src[0] if src.dim() == 4 and src.shape[0] == 1 else src
        if src.dim() != 3 or src.shape[0] != 3:
            raise _lib.DawnHipError("MotionEvaluator: an fp32 source image is (3,H,W) or (1,3,H,W)")
        return src.float().contiguous(), 0, int(src.shape[1]), int(src.shape[2])

    @staticmethod
    def _driving(drv: Tensor, H: int, W: int):
        """-> (tensor kept alive, kind, T, frame stride, channel stride): fp32 (T,3,H,W) with dense planes (a (3,T,H,W) clip permuted is
        taken as it is), uint8 (T,H,W,3) contiguous, or uint8 (T, >= 3HW/2) I420 rows."""
        if drv.dtype == torch.uint8 and drv.dim() == 2:
            if drv.stride(1) != 1 or drv.shape[1] < H * W * 3 // 2:
                raise _lib.DawnHipError("MotionEvaluator: I420 driving frames are uint8 (T, >= 3*H*W/2) rows")
            T = int(drv.shape[0])
            return drv, 2, T, (int(drv.stride(0)) if T > 1 else int(drv.shape[1])), 0
        if drv.dtype == torch.uint8:
            if drv.dim() != 4 or tuple(drv.shape[1:]) != (H, W, 3):
                raise _lib.DawnHipError("MotionEvaluator: uint8 driving frames are (T,H,W,3) of the source's size")
            return drv.contiguous(), 1, int(drv.shape[0]), H * W * 3, 1
        if drv.dim() != 4 or tuple(drv.shape[1:]) != (3, H, W):
            raise _lib.DawnHipError("MotionEvaluator: fp32 driving frames are (T,3,H,W) of the source's size")
        drv = drv.float()
        if not (drv.stride(3) == 1 and drv.stride(2) == W):
            drv = drv.contiguous()
        T = int(drv.shape[0])
        return drv, 0, T, (int(drv.stride(0)) if T > 1 else 3 * H * W), int(drv.stride(1))

    def encode_into(self, src: Tensor, drv: Tensor, grid: Tensor, conf: Tensor, chunk: int = 16, conf_x0: bool = False,
                    workspace: Optional[Tensor] = None) -> None:
        """dawn_motion_encode_clip into grid (2,T,h,w) (dense planes, any plane stride) and conf (T,h,w) contiguous."""
        s, sk, H, W = self._source(src)
        d, dk, T, fs, cs = self._driving(drv, H, W)
        h, w = self.latent_size(H, W)
        for t in (s, d, grid, conf):
            if not t.is_cuda:
                raise _lib.DawnHipError("MotionEvaluator needs GPU tensors; there is no CPU fallback on the product path")
        if not (grid.dtype == torch.float32 and tuple(grid.shape) == (2, T, h, w) and grid.stride(3) == 1 and grid.stride(2) == w and grid.stride(1) == h * w):
            raise _lib.DawnHipError(f"MotionEvaluator: grid must be fp32 (2,{T},{h},{w}) with dense planes")
        if not (conf.dtype == torch.float32 and tuple(conf.shape) == (T, h, w) and conf.is_contiguous()):
            raise _lib.DawnHipError(f"MotionEvaluator: conf must be fp32 ({T},{h},{w}) contiguous")
        chunk = max(1, min(int(chunk), T))
        ws = workspace if workspace is not None else self.workspace(H, W, chunk)
        with torch.cuda.device(self.device):
            check(self.L.dawn_motion_encode_clip(self.h, H, W, T, s.data_ptr(), sk, d.data_ptr(), dk, fs, cs, chunk, grid.data_ptr(), grid.stride(0),
                                                 conf.data_ptr(), 1 if conf_x0 else 0, ws.data_ptr(), ws.numel(), self._stream()),
                  "dawn_motion_encode_clip")

    def encode_clip(self, src: Tensor, drv: Tensor, chunk: int = 16, workspace: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """MotionEncoder.encode_clip through the C stage: -> {real_vid_grid (1,2,T,h,w), real_vid_conf (1,1,T,h,w)}."""
        _, _, H, W = self._source(src)
        T = int(drv.shape[0])
        h, w = self.latent_size(H, W)
        grid = torch.empty(2, T, h, w, device=self.device, dtype=torch.float32)
        conf = torch.empty(T, h, w, device=self.device, dtype=torch.float32)
        self.encode_into(src, drv, grid, conf, chunk, False, workspace)
        return {"real_vid_grid": grid.unsqueeze(0), "real_vid_conf": conf.view(1, 1, T, h, w)}

    def latent(self, src: Tensor, drv: Tensor, chunk: int = 16, workspace: Optional[Tensor] = None) -> Tensor:
        """-> (3,T,h,w): the diffusion's x0 of this clip, cat(grid, 2 * conf - 1)."""
        _, _, H, W = self._source(src)
        T = int(drv.shape[0])
        h, w = self.latent_size(H, W)
        lat = torch.empty(3, T, h, w, device=self.device, dtype=torch.float32)
        self.encode_into(src, drv, lat[:2], lat[2], chunk, True, workspace)
        return lat

    def reenact(self, decoder, src: Tensor, drv: Tensor, *, format: str = "rgb", mean=(0.0, 0.0, 0.0), bgr: bool = False, motion_chunk: int = 16,
                chunk: int = 64, want_motion: bool = False, workspace: Optional[Tensor] = None):
        """dawn_reenact_clip: src fp32 (3,H,W) / (1,3,H,W), drv as encode_clip, `decoder` a DecoderEvaluator (or anything with its
        handle as `.h`) -> (T,H,W,3) uint8 frames, or (T, 3HW/2) with format="yuv420p"; want_motion: -> (frames, grid (2,T,h,w),
        conf (T,h,w))."""
        if format not in ("rgb", "yuv420p"):
            raise ValueError(f"format must be 'rgb' or 'yuv420p', not {format!r}")
        s, sk, H, W = self._source(src)
        if sk != 0:
            raise _lib.DawnHipError("MotionEvaluator.reenact: the source image is fp32 (3,H,W): the decoder reads it too")
        d, dk, T, fs, cs = self._driving(drv, H, W)
        h, w = self.latent_size(H, W)
        a = ReenactArgs()
        a.size, a.motion, a.decoder, a.img3, a.H, a.W = C.sizeof(ReenactArgs), self.h, decoder.h, s.data_ptr(), H, W
        a.drv, a.drv_kind, a.T, a.drv_frame_stride, a.drv_chan_stride = d.data_ptr(), dk, T, fs, cs
        a.motion_chunk, a.chunk = max(1, min(int(motion_chunk), T)), max(1, min(int(chunk), T))
        a.format, a.bgr = (1 if format == "yuv420p" else 0), (1 if bgr else 0)
        m = (C.c_double * 3)(*[float(v) / 255.0 for v in mean])
        a.mean3 = C.cast(m, C.POINTER(C.c_double))
        grid = conf = None
        if want_motion:
            grid = torch.empty(2, T, h, w, device=self.device, dtype=torch.float32)
            conf = torch.empty(T, h, w, device=self.device, dtype=torch.float32)
            a.grid_out, a.conf_out = grid.data_ptr(), conf.data_ptr()
        cb, wb = C.c_size_t(0), C.c_size_t(0)
        check(self.L.dawn_reenact_bytes(C.addressof(a), C.byref(cb), C.byref(wb)), "dawn_reenact_bytes")
        frames = torch.empty(cb.value, dtype=torch.uint8, device=self.device)
        a.frames_out = frames.data_ptr()
        ws = workspace if workspace is not None else self._grown(wb.value)
        with torch.cuda.device(self.device):
            check(self.L.dawn_reenact_clip(C.addressof(a), ws.data_ptr(), ws.numel(), self._stream()), "dawn_reenact_clip")
        frames = frames.view(T, H * W * 3 // 2) if format == "yuv420p" else frames.view(T, H, W, 3)
        return (frames, grid, conf) if want_motion else frames


# ---------------------------------------------------------------------------------------------------------------------
# the same pipeline from a model bundle file (include/dawn_hip.h: "model bundle"; csrc/dawn_bundle.hip): what a host without Python does
class _BundleStage:
    """What PipelineEvaluator asks of a stage evaluator: the handle and the cfg struct (the bundle owns handles and weights)."""

    def __init__(self, h, cfg, device):
        self.h, self.cfg, self.device = h, cfg, device


class BundleEvaluator(PipelineEvaluator):
    """PipelineEvaluator whose six handles come from a bundle file through the C loader: dawn_bundle_open -> upload into one torch uint8
    tensor (`mem`) -> verify on the device -> dawn_bundle_create_handles.  The same `args / sizes / generate / from_media / media_sizes /
    generate_media` surface, plus `steps(name)`, `defaults()`, `cfg(stage)`, `table(stage)` and `tensor(stage, name)` (the uploaded
    bytes of one entry)."""

    def __init__(self, path, device="cuda:0", verify: bool = True):
        from . import bundle
        self.L = _lib.lib()
        self.device = torch.device(device)
        self.path = os.fspath(path)
        self.b, self._args = None, None
        b = C.c_void_p()
        check(self.L.dawn_bundle_open(self.path.encode(), C.addressof(b)), "dawn_bundle_open")
        self.b = b
        self.index = bundle.read_index(self.path)
        with torch.cuda.device(self.device):
            self.mem = torch.empty(max(int(self.L.dawn_bundle_device_bytes(self.b)), 1), dtype=torch.uint8, device=self.device)
            check(self.L.dawn_bundle_upload(self.b, self.mem.data_ptr(), self.mem.numel(), _Evaluator._stream()), "dawn_bundle_upload")
            if verify:
                self.verify()
            a = GenerateArgs()
            check(self.L.dawn_bundle_create_handles(self.b, self.mem.data_ptr(), C.addressof(a)), "dawn_bundle_create_handles")
        self._args = a
        cfgs = (HubertCfg, PbnetCfg, PbnetCfg, DecoderCfg, InputsCfg, UnetCfg)
        handles = (a.hubert, a.pose, a.blink, a.decoder, a.inputs, a.unet)
        self.ev = tuple(_BundleStage(h, self.cfg(s, cls), self.device) for s, (h, cls) in enumerate(zip(handles, cfgs)))
        self._ws: Optional[Tensor] = None

    def __del__(self):
        a, self._args = getattr(self, "_args", None), None
        if a is not None:
            self.L.dawn_bundle_destroy_handles(C.addressof(a))
        b, self.b = getattr(self, "b", None), None
        if b:
            self.L.dawn_bundle_close(b)

    def verify(self, workspace: Optional[Tensor] = None) -> None:
        """dawn_bundle_verify of `mem`; raises DawnHipError naming the first failing stage and tensor."""
        if workspace is None:
            workspace = torch.empty(int(self.L.dawn_bundle_verify_workspace_bytes(self.b)), dtype=torch.uint8, device=self.device)
        check(self.L.dawn_bundle_verify(self.b, self.mem.data_ptr(), self.mem.numel(), workspace.data_ptr(), workspace.numel(),
                                        _Evaluator._stream()), "dawn_bundle_verify")

    def cfg(self, stage: int, cls):
        out = cls()
        check(self.L.dawn_bundle_cfg(self.b, stage, C.addressof(out), C.sizeof(out)), "dawn_bundle_cfg")
        return out

    def host(self, name: str) -> bytes:
        p, n = C.c_void_p(), C.c_size_t(0)
        check(self.L.dawn_bundle_host(self.b, name.encode(), C.addressof(p), C.byref(n)), "dawn_bundle_host")
        return C.string_at(p.value, n.value)

    def steps(self, name: str) -> List[dict]:
        """The step table "steps.<name>" ("ddim.20", "ancestral.1000") as the dicts `args(...)` takes."""
        raw = self.host(f"steps.{name}")
        cls = AncestralStep if name.startswith("ancestral.") else DdimStep
        arr = (cls * (len(raw) // C.sizeof(cls))).from_buffer_copy(raw)
        return [{f: getattr(s, f) for f, _ in cls._fields_} for s in arr]

    def defaults(self):
        from .bundle import Defaults
        return Defaults.from_buffer_copy(self.host("defaults"))

    def motion(self) -> "MotionEvaluator":
        """The motion-encode stage of the bundle (dawn_bundle_create_motion) as a MotionEvaluator on the bundle's region; DawnHipError
        "stage 'motion' is missing" for a bundle without it.  The evaluator owns its handle and keeps this bundle alive."""
        m = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.dawn_bundle_create_motion(self.b, self.mem.data_ptr(), C.addressof(m)), "dawn_bundle_create_motion")
        return MotionEvaluator(handle=m, cfg=self.cfg(7, MotionCfg), device=self.device, keep=self)

    def table(self, stage: int) -> Dict[str, int]:
        """{name: device address} of dawn_bundle_table for `mem`."""
        t, n = C.c_void_p(), C.c_int(0)
        check(self.L.dawn_bundle_table(self.b, stage, self.mem.data_ptr(), C.addressof(t), C.byref(n)), "dawn_bundle_table")
        arr = C.cast(t, C.POINTER(NamedPtr))
        return {arr[i].name.decode(): int(arr[i].ptr) for i in range(n.value)}

    def tensor(self, stage: str, name: str) -> Tensor:
        """The uploaded bytes of one device entry (its zero padding to whole words included): a view of `mem`."""
        for e in self.index["entries"]:
            if e["kind"] == 0 and e["stage"] == stage and e["name"] == name:
                return self.mem[e["offset"]:e["offset"] + e["length"]]
        raise KeyError(f"{stage}/{name}")
