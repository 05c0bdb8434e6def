"""Known-frame conditioning and the chunk plan without a GPU.  The replacement is not in the reference: its values are the definition
written in include/dawn_hip.h.  The host's noise levels equal an fp64 recomputation; sampler.chunk_plan and the library's dawn_chunk_plan
agree and tile the clip; the Python loop on the torch reference op set equals a loop restated plainly here (the evaluation, the existing
x0 / threshold / update ops, the replacement as defined) bit for bit, for DDIM, ancestral and DPM-Solver++(2M) in every clip mode; the
new C-ABI names exist and are bound."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT, load_golden
from oracle.ops_ref import RefOps
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib, abi
from dawn_pytorch_amd import sampler as SM
from dawn_pytorch_amd.sampler import cosine_schedule_buffers

T = torch.from_numpy
TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3)
S_TINY = 6
KNOWN = (0, 1, 2, 11)                  # both ends of the 12-frame clip pinned
MODES = {"dynamic": ("dynamic", 0.9), "static": ("static",), "none": ("none",)}
NEW = {"dawn_known_replace", "dawn_sampler_run_known", "dawn_chunk_plan"}


def known_replace_ref(x, known, mask, a, b, z):
    """The definition: x[:, f] = fadd(fmul(a, known[:, f]), fmul(b, z[:, f])) on the frames with mask[f] != 0, every operation rounded
    to fp32 on its own (torch on the CPU does not contract); b == 0: x = fmul(a, known), z is not read."""
    m = mask != 0
    v = torch.tensor(a, dtype=torch.float32) * known[:, m]
    if b != 0.0:
        v = v + torch.tensor(b, dtype=torch.float32) * z[:, m]
    x[:, m] = v
    return x


class KnownRefOps(RefOps):
    """The reference op set plus the fused step tails of the other clip modes and solvers in plain torch, and the replacement as defined."""

    def with_comm(self, comm):
        return KnownRefOps(comm)

    def cfg_x0(self, e_null, e_cond, scale, x, recip, recipm1):
        eps = self.cfg_combine(e_null, e_cond, scale)
        x0, hist = self.ddim_x0(x, eps, recip, recipm1)
        return eps, x0, hist

    def ddim_step_fixed(self, x, eps, noise, recip, recipm1, sqrt_alpha_next, c, sigma, clamp=True):
        x0 = recip * x - recipm1 * eps
        out = (x0.clamp(-1., 1.) if clamp else x0) * sqrt_alpha_next + c * eps
        return out if noise is None else out + sigma * noise

    def ancestral_update(self, x0, x_t, s, noise, c1, c2, std):
        return self.ddim_update(x0, x_t, s, noise, c1, c2, std)

    def ancestral_step_fixed(self, x_t, eps, noise, recip, recipm1, c1, c2, std, clamp=True):
        x0 = recip * x_t - recipm1 * eps
        out = x0.clamp(-1., 1.) * c1 + c2 * x_t
        return out if noise is None else out + std * noise

    @staticmethod
    def _tail(x, v, v_prev, a, b, c, v_out):
        out = a * x + b * v
        if v_prev is not None:
            out = out + c * v_prev
        if v_out is None:
            v_out = torch.full_like(v, float("nan"))
        v_out.copy_(v)
        return out, v_out

    def dpmpp_update(self, x0, s, x, v_prev, a, b, c, v_out=None, out=None):
        sv = s[0]
        return self._tail(x, torch.minimum(torch.maximum(x0, -sv), sv) / sv, v_prev, a, b, c, v_out)

    def dpmpp_step_fixed(self, x, eps, v_prev, recip, recipm1, a, b, c, clamp=True, v_out=None, out=None):
        x0 = recip * x - recipm1 * eps
        return self._tail(x, x0.clamp(-1., 1.) if clamp else x0, v_prev, a, b, c, v_out)

    def known_replace(self, x, known, mask, a, b, noise=None, seed=0, stream_id=0, f0=0, Ftotal=None, out=None):
        if out is not None:
            out.copy_(x)
            x = out
        z = noise
        if z is None and b != 0.0:
            F = x.shape[1]
            z = self.philox_normal(3, F, f0, F if Ftotal is None else Ftotal, x[0, 0].numel(), seed, stream_id, x.device).reshape(x.shape)
        return known_replace_ref(x, known, mask, a, b, z)


# ------------------------------------------------------------------------------------------------------------ 1. ABI
def test_known_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NEW <= set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src))
    assert NEW <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
    assert L.dawn_abi_version() == 8                       # additive: nothing that existed changed layout or meaning
    assert len(abi.structs(text)) == 18                    # levels and noises travel as plain arrays: no new struct
    assert re.search(r"enum \{ DAWN_SOLVER_DDIM = 0, DAWN_SOLVER_ANCESTRAL = 1, DAWN_SOLVER_DPMPP = 2 \};", src)
    assert len(set(re.findall(r"\bDAWN_OPT_[A-Z_]+", src))) == 7
    from dawn_pytorch_amd import ctx
    assert (ctx.SOLVER_DDIM, ctx.SOLVER_ANCESTRAL, ctx.SOLVER_DPMPP) == (0, 1, 2)
    import inspect
    for name in ("sample", "sample_ancestral", "sample_dpmpp"):
        assert "known" in inspect.signature(getattr(ctx.CtxEvaluator, name)).parameters, name
    from dawn_pytorch_amd.ops import HipOps
    assert hasattr(HipOps, "known_replace")
    for name in ("sample", "ddim_sample", "p_sample_loop"):
        p = inspect.signature(getattr(D.GaussianDiffusion, name)).parameters
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("known_latent", "known_mask", "known_noises")), name


# ------------------------------------------------------------------------------------------------------------ 2. levels
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float64).float())


@pytest.mark.parametrize("kind", ["ddim", "dpmpp", "ancestral"])
def test_known_level_scalars_equal_an_fp64_recomputation(kind):
    bufs = cosine_schedule_buffers(1000)
    prev, acp = bufs["alphas_cumprod_prev"], bufs["alphas_cumprod"]
    assert prev.dtype == torch.float32 and float(prev[0]) == 1.0
    if kind == "ancestral":
        steps = SM.ancestral_step_scalars(bufs, 1000)
        abars = [float(acp[999])] + [float(prev[st["t"]]) for st in steps]
        assert [st["t"] for st in steps] == list(range(999, -1, -1))
    else:
        steps = SM.ddim_step_scalars(bufs, S_TINY, 1.0) if kind == "ddim" else SM.dpmpp_step_scalars(bufs, S_TINY)
        pairs = SM.ddim_time_pairs(S_TINY, 1000)
        abars = [float(prev[pairs[0][0]])] + [float(prev[tn]) for _, tn in pairs]
    levels = SM.known_level_scalars(bufs, steps, kind, 1000)
    assert len(levels) == len(steps) + 1
    for (a, b), ab in zip(levels, abars):
        assert a == _f32(math.sqrt(ab)) and b == _f32(math.sqrt(1.0 - ab)), (a, b, ab)
        assert _f32(a) == a and _f32(b) == b                # already fp32 values
    assert levels[-1] == (1.0, 0.0)
    a0, b0 = levels[0]
    assert 0.0 < a0 < 0.25 and 0.97 < b0 <= 1.0            # level 0 is almost pure noise
    if kind != "ancestral":                                 # ... and the level the DDIM loop itself starts from (MT:1170)
        assert a0 == _f32(math.sqrt(float(prev[steps[0]["t"]])))
    assert all(x[0] <= y[0] and x[1] >= y[1] for x, y in zip(levels, levels[1:]))
    with pytest.raises(ValueError, match="unknown sampler step kind"):
        SM.known_level_scalars(bufs, steps, "plms")


# ------------------------------------------------------------------------------------------------------------ 3. chunk plan
def _c_plan(T_, F, K):
    L = _lib.lib()
    n = L.dawn_chunk_plan(T_, F, K, None, None, 0)
    if n < 0:
        return None
    st, kn = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    assert L.dawn_chunk_plan(T_, F, K, st, kn, n) == n
    return [(st[i], min(F, T_), kn[i]) for i in range(n)]


SWEEP = [(T_, F, K) for F in (2, 3, 5, 8, 12, 56) for K in sorted({1, 2, F // 2, F - 1}) if 1 <= K < F
         for T_ in sorted({1, F - 1, F, F + 1, F + 2, 2 * F - K, 2 * F - K + 1, K + 3 * (F - K), K + 4 * (F - K), 5 * F + 3, 200}) if T_ >= 1]


def test_chunk_plan_python_and_c_agree_and_tile_the_clip():
    assert (30, 12, 4) not in SWEEP and len(SWEEP) > 150
    assert any(T_ < F for T_, F, K in SWEEP) and any(T_ == F for T_, F, K in SWEEP) and any(T_ == F + 1 for T_, F, K in SWEEP)
    assert any(K == F - 1 and T_ > F for T_, F, K in SWEEP) and any(T_ > F and (T_ - K) % (F - K) == 0 for T_, F, K in SWEEP)
    for T_, F, K in SWEEP + [(30, 12, 4)]:
        plan = SM.chunk_plan(T_, F, K)
        assert plan == _c_plan(T_, F, K), (T_, F, K)
        if T_ <= F:
            assert plan == [(0, T_, 0)]
            continue
        assert all(n == F for _, n, _ in plan) and plan[0] == (0, F, 0)
        assert all(kn >= K for _, _, kn in plan[1:]) and all(kn == K for _, _, kn in plan[1:-1]) and K <= plan[-1][2] <= F - 1
        assert [s for s, _, _ in plan[:-1]] == list(range(0, plan[-2][0] + 1, F - K)) and plan[-1][0] == T_ - F
        assert plan[-2][0] + F < T_ <= plan[-2][0] + F - K + F          # the last regular chunk stops short, one more reaches the end
        emitted = [f for s, n, kn in plan for f in range(s + kn, s + n)]
        assert emitted == list(range(T_)), (T_, F, K)                     # disjoint, in order, covering the clip
        covered = set()
        for s, n, kn in plan:                                            # the known frames of a chunk are generated already
            assert set(range(s, s + kn)) <= covered, (T_, F, K)
            covered |= set(range(s, s + n))
    assert SM.chunk_plan(30, 12, 4) == [(0, 12, 0), (8, 12, 4), (16, 12, 4), (18, 12, 10)]


@pytest.mark.parametrize("T_,F,K", [(30, 12, 0), (30, 12, 12), (30, 12, 13), (30, 12, -1), (30, 1, 1), (0, 12, 4)])
def test_chunk_plan_refuses_a_bad_overlap(T_, F, K):
    with pytest.raises(ValueError, match="chunk_plan"):
        SM.chunk_plan(T_, F, K)
    L = _lib.lib()
    assert L.dawn_chunk_plan(T_, F, K, None, None, 0) < 0
    assert b"dawn_chunk_plan" in L.dawn_last_error()


# ------------------------------------------------------------------------------------------------------------ 4. the loop
def _tiny_diffusion(sd, mode, ops, S=S_TINY, T_=12, timesteps=1000):
    unet = D.DynamicNfUnet3D(default_num_frames=T_, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    unet.ops = ops
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=8, sampling_timesteps=S,
                                        timesteps=timesteps, loss_type='l2', null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw)
    diff.update_num_frames(T_)
    unet.update_num_frames(T_)
    return unet, diff


def _inputs():
    d = load_golden("ddim_tiny.npz")
    g = torch.Generator().manual_seed(20)
    noises = [torch.randn(1, 3, 12, 8, 8, generator=g) for _ in range(S_TINY)]
    known_noises = [torch.randn(1, 3, 12, 8, 8, generator=g) for _ in range(S_TINY + 1)]
    known = torch.randn(1, 3, 12, 8, 8, generator=g).clamp(-1., 1.)
    mask = torch.zeros(12, dtype=torch.uint8)
    mask[list(KNOWN)] = 1
    return d, noises, known_noises, known, mask


def restated_loop(unet, steps, levels, kind, mode, d, scale, noises, known, mask, known_z):
    """The loop, plainly: per step the evaluation, the existing x0 / threshold / update ops, then the replacement as defined.
    known = None: the plain sampler.  known_z(i) -> z_i."""
    ops, P = unet._ops(), unet.packed()
    fea = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)[0].contiguous()
    cond = T(d["cond"])[0].contiguous()
    cs = unet.build_clip(fea, cond)
    csn = unet.build_clip(fea, torch.zeros_like(cond)) if scale != 1.0 else None
    x = T(d["x_init"])[0].clone()
    if known is not None:
        x = known_replace_ref(x, known, mask, *levels[0], known_z(0))
    v_prev = None
    for i, st in enumerate(steps):
        if scale != 1.0:
            e_c, e_n = SM.unet_forward_guided(ops, P, cs, csn, x, st["t"])
            eps = ops.cfg_combine(e_n, e_c, scale)
        else:
            eps = SM.unet_forward(ops, P, cs, x, st["t"])
        x0, hist = ops.ddim_x0(x, eps, st["recip"], st["recipm1"])
        if mode[0] == "dynamic":
            s = ops.quantile_threshold(x0, hist, x0.numel(), mode[1])
            v = torch.minimum(torch.maximum(x0, -s[0]), s[0]) / s[0]
        else:
            v = x0.clamp(-1., 1.) if mode[0] == "static" else x0
        if kind == "dpmpp":
            nxt = st["a"] * x + st["b"] * v
            if st["c"] != 0.0:
                nxt = nxt + st["c"] * v_prev
            x, v_prev = nxt, v
        elif kind == "ancestral":
            nxt = v * st["c1"] + st["c2"] * x
            x = nxt + st["std"] * noises[i][0] if st["t"] > 0 else nxt
        else:
            nxt = v * st["sqrt_alpha_next"] + st["c"] * eps
            x = nxt + st["sigma"] * noises[i][0] if st["t_next"] > 0 else nxt
        if known is not None:
            x = known_replace_ref(x, known, mask, *levels[i + 1], known_z(i + 1))
    return x


CASES = [("ddim", m) for m in sorted(MODES)] + [("ancestral", "dynamic"), ("ancestral", "static")] + [("dpmpp", m) for m in sorted(MODES)]


@pytest.mark.parametrize("kind,mode_name", CASES)
def test_loop_equals_the_restated_definition(tiny, kind, mode_name):
    """S = 6 on the tiny UNet, known frames {0, 1, 2, 11}, injected step noise and injected known-frame noise.  DDIM and DPM-Solver++
    through GaussianDiffusion.sample / ddim_sample; the ancestral loop through sampler.ancestral_sample_clip on the LAST six of its
    1000 steps with the last seven of its levels (the full loop is 1000 evaluations)."""
    _, sd = tiny
    mode = MODES[mode_name]
    d, noises, kz, known, mask = _inputs()
    unet, diff = _tiny_diffusion(sd, mode, KnownRefOps())
    bufs = cosine_schedule_buffers(1000)
    if kind == "ancestral":
        steps = SM.ancestral_step_scalars(bufs, 1000)[-S_TINY:]
        levels = SM.known_level_scalars(bufs, SM.ancestral_step_scalars(bufs, 1000), "ancestral", 1000)[-(S_TINY + 1):]
        assert levels[0] == (_f32(math.sqrt(float(bufs["alphas_cumprod"][5]))), _f32(math.sqrt(1.0 - float(bufs["alphas_cumprod"][5]))))
    else:
        steps = SM.ddim_step_scalars(bufs, S_TINY, 1.0) if kind == "ddim" else SM.dpmpp_step_scalars(bufs, S_TINY)
        levels = SM.known_level_scalars(bufs, steps, kind, 1000)
        diff.solver = "dpmpp2m" if kind == "dpmpp" else "ddim"

    def run(known_latent, known_mask, known_noises):
        if kind == "ancestral":
            fea = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)[0].contiguous()
            cs = unet.build_clip(fea, T(d["cond"])[0].contiguous())
            kf = None
            if known_latent is not None:
                kf = SM.KnownFrames(known_latent[0], known_mask, levels, None if known_noises is None else (lambda i: known_noises[i][0]))
            return SM.ancestral_sample_clip(unet._ops(), unet.packed(), cs, T(d["x_init"])[0], steps, lambda i: noises[i][0], clip=mode,
                                            known=kf)[None]
        kw = dict(cond=T(d["cond"]), x_init=T(d["x_init"]), noises=noises, known_latent=known_latent, known_mask=known_mask,
                  known_noises=known_noises)
        if mode[0] == "none":
            return diff.ddim_sample(torch.cat([T(d["fea"]), T(d["bbox"])], dim=1), (1, 3, 12, 8, 8), clip_denoised=False, **kw)
        return diff.sample(T(d["fea"]), T(d["bbox"]), **kw)

    x_init_before = T(d["x_init"]).clone()
    out = run(known, mask, kz)
    want = restated_loop(unet, steps, levels, kind, mode, d, 1.0, noises, known[0], mask, lambda i: kz[i][0])
    assert torch.equal(out[0], want)
    assert torch.equal(T(d["x_init"]), x_init_before)                                   # level 0 works on a copy
    m = mask.bool()
    assert torch.equal(out[0][:, m], known[0][:, m])                                    # the known frames, bit for bit
    assert not torch.equal(out[0][:, ~m], known[0][:, ~m])
    plain = run(None, None, None)
    assert torch.equal(plain[0], restated_loop(unet, steps, levels, kind, mode, d, 1.0, noises, None, None, None))
    zero = run(known, torch.zeros(12, dtype=torch.uint8), kz)
    assert torch.equal(zero, plain)                                                     # an empty known set changes nothing
    assert not torch.allclose(out[0][:, ~m], plain[0][:, ~m], atol=1e-3)                # the free frames were generated to fit
    ones = run(known, torch.ones(12, dtype=torch.uint8), kz)
    assert torch.equal(ones, known)                                                     # everything known: the known latent


def test_guided_seeded_and_batched_mask(tiny):
    """cond_scale = 2.5, the known-frame noise from the counter-based generator (noise_seed; RefOps restates the generator bit for bit),
    and a (B, T) mask: equal to the restated loop with z_i = philox_normal(seed, 0x80000000 + i)."""
    _, sd = tiny
    mode = MODES["dynamic"]
    d, noises, _, known, mask = _inputs()
    unet, diff = _tiny_diffusion(sd, mode, KnownRefOps())
    diff.noise_seed = 77
    bufs = cosine_schedule_buffers(1000)
    steps = SM.ddim_step_scalars(bufs, S_TINY, 1.0)
    levels = SM.known_level_scalars(bufs, steps, "ddim", 1000)
    ops = KnownRefOps()
    z = lambda i: ops.philox_normal(3, 12, 0, 12, 64, 77, 0x80000000 + i, "cpu").reshape(3, 12, 8, 8)      # noqa: E731
    out = diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), cond_scale=2.5, x_init=T(d["x_init"]), noises=noises,
                      known_latent=known, known_mask=mask[None])
    want = restated_loop(unet, steps, levels, "ddim", mode, d, 2.5, noises, known[0], mask, z)
    assert torch.equal(out[0], want)
    assert SM.KNOWN_STREAM0 == 0x80000000 and SM.KNOWN_STREAM0 + S_TINY < 0xFFFFFFFE       # disjoint from the step streams and PBnet's


def test_full_ancestral_loop_takes_the_keywords(tiny, monkeypatch):
    """p_sample_loop with a known set over all 1000 steps (the evaluation stubbed): 1001 levels, the result holds the known frames."""
    _, sd = tiny
    d, _, _, known, mask = _inputs()
    _, diff = _tiny_diffusion(sd, MODES["dynamic"], KnownRefOps(), S=1000)
    assert not diff.is_ddim_sampling
    diff.noise_seed = 3
    calls = []
    monkeypatch.setattr(SM, "unet_forward", lambda ops, P, cs, x, t, **k: (calls.append(t), torch.zeros_like(x))[1])
    out = diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), x_init=T(d["x_init"]), known_latent=known, known_mask=mask)
    assert calls == list(range(999, -1, -1))
    m = mask.bool()
    assert torch.equal(out[0][:, m], known[0][:, m]) and bool(torch.isfinite(out).all())


def test_keyword_validation(tiny):
    _, sd = tiny
    d, noises, kz, known, mask = _inputs()
    _, diff = _tiny_diffusion(sd, MODES["dynamic"], KnownRefOps())
    kw = dict(cond=T(d["cond"]), x_init=T(d["x_init"]), noises=noises)
    with pytest.raises(ValueError, match="known_latent needs known_mask"):
        diff.sample(T(d["fea"]), T(d["bbox"]), known_latent=known, **kw)
    with pytest.raises(ValueError, match="need known_latent"):
        diff.sample(T(d["fea"]), T(d["bbox"]), known_mask=mask, **kw)
    with pytest.raises(ValueError, match="known_latent must be"):
        diff.sample(T(d["fea"]), T(d["bbox"]), known_latent=known[:, :, :5], known_mask=mask, **kw)
    with pytest.raises(ValueError, match="known_mask must be"):
        diff.sample(T(d["fea"]), T(d["bbox"]), known_latent=known, known_mask=mask[:5], **kw)
    with pytest.raises(ValueError, match="known_noises"):
        diff.sample(T(d["fea"]), T(d["bbox"]), known_latent=known, known_mask=mask, known_noises=kz[:3], **kw)


# ------------------------------------------------------------------------------------------------------------ 5. chunked driver
def test_chunked_driver_on_the_reference_ops(tiny):
    """T = 30, F = 12, K = 4 on the CPU op set: sample_chunked equals the hand-written loop of sample(known_...) calls, iter_chunks
    yields the same frames in order, overlapping frames are bit-identical in both chunks, the attributes are restored, and a T-shard
    communicator is refused."""
    _, sd = tiny
    unet, diff = _tiny_diffusion(sd, MODES["dynamic"], KnownRefOps(), S=3)
    diff.noise_seed = 5
    g = torch.Generator().manual_seed(4)
    fea, bbox, cond = torch.randn(1, 12, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, 30, 32, generator=g)
    whole = diff.sample_chunked(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4)
    assert whole.shape == (1, 3, 30, 8, 8) and diff.num_frames == 12 and diff.noise_seed == 5
    chunks, prev, prev_start = [], None, 0
    for j, (start, n, kn) in enumerate(SM.chunk_plan(30, 12, 4)):
        diff.noise_seed = 5 + (j << 32)
        kl = km = None
        if kn:
            kl = torch.zeros(1, 3, 12, 8, 8)
            kl[:, :, :kn] = prev[:, :, start - prev_start:start - prev_start + kn]
            km = torch.cat([torch.ones(kn, dtype=torch.uint8), torch.zeros(12 - kn, dtype=torch.uint8)])
        out = diff.sample(fea, bbox, cond=cond[:, start:start + n].contiguous(), known_latent=kl, known_mask=km)
        if kn:
            assert torch.equal(out[:, :, :kn], prev[:, :, start - prev_start:start - prev_start + kn])      # the overlap, bit for bit
        chunks.append((start + kn, out[:, :, kn:]))
        prev, prev_start = out, start
    diff.noise_seed = 5
    assert torch.equal(whole, torch.cat([c for _, c in chunks], dim=2))
    got = list(diff.iter_chunks(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4))
    assert [f for f, _ in got] == [f for f, _ in chunks] == [0, 12, 20, 28]
    assert all(torch.equal(a, b) for (_, a), (_, b) in zip(got, chunks))
    diff.update_num_frames(10)
    short = diff.sample_chunked(fea, bbox, cond[:, :10].contiguous(), 1.0, chunk_frames=12, overlap=4)
    assert torch.equal(short, diff.sample(fea, bbox, cond=cond[:, :10].contiguous()))
    with pytest.raises(ValueError, match="T-shard"):
        diff.iter_chunks(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4, comm=object())
    with pytest.raises(ValueError, match="chunk_plan"):
        diff.sample_chunked(fea, bbox, cond, 1.0, chunk_frames=12, overlap=12)


def test_flow_diffusion_samples_in_chunks_when_asked(monkeypatch):
    """FlowDiffusion.chunk_frames / chunk_overlap (plain attributes, like diffusion.solver): sample_one_video runs the pre / sample /
    post path with the 5-frame clip sampled as chunks of 3 with overlap 1 (the evaluation stubbed), the decode after it unchanged."""
    import inspect
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    from test_boundary_cpu import FakeLFG
    assert not {"chunk_frames", "chunk_overlap"} & set(inspect.signature(FlowDiffusion.__init__).parameters)
    fd = FlowDiffusion(generator=FakeLFG(), pose_dim=6, sampling_timesteps=2, win_width=40, num_frames=5, img_size=16)
    assert fd.chunk_frames is None and fd.chunk_overlap == 0
    fd.unet.ops = KnownRefOps()
    fd.update_num_frames(5)
    fd.diffusion.noise_seed = 2
    frames = []
    monkeypatch.setattr(SM, "unet_forward", lambda ops, P, cs, x, t, **k: (frames.append(x.shape[1]), 0.1 * x)[1])
    d = load_golden("fd_prepost.npz")
    args = (T(d["img"]), T(d["hubert"]), T(d["pose"]), T(d["eye"]), T(d["bbox"]), 1.0)
    kw = dict(init_pose=T(d["init_pose"]), init_eye=T(d["init_eye"]))
    whole = fd.sample_one_video(*args, **kw)
    assert frames == [5] * 4                                                            # two clips, two steps
    frames.clear()
    fd.chunk_frames, fd.chunk_overlap = 3, 1
    out = fd.sample_one_video(*args, **kw)
    assert SM.chunk_plan(5, 3, 1) == [(0, 3, 0), (2, 3, 1)] and frames == [3] * 8       # two chunks of three frames, B = 2, two steps
    assert fd.diffusion.num_frames == 5 and fd.diffusion.noise_seed == 2
    for k in ("sample_vid_grid", "sample_vid_conf", "sample_out_vid"):
        assert out[k].shape == whole[k].shape and bool(torch.isfinite(out[k]).all()), k
