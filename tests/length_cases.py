"""Clip lengths at which one UNet evaluation mixes kernels, shared by tools/gen_goldens_lengths.py (CPU: writes
tests/golden/length_F{F}_h{h}.npz from the project's float64 oracle) and the tests that consume those fixtures
(tests/test_length_gate_cpu.py, tests/test_hip_length_gates.py), in the manner of fullsize_cases.py.

The clip length F comes from the audio, so it is arbitrary, and the library's routers choose the kernel of every conv / GEMM from
M = F x rows per frame: the split 1x1 kernels need M % 256 == 0 and M >= 6400, the resample form M >= 12800, both Winograd forms and the
direct split 3x3 kernel M % 256 == 0.  At latent side 32 the levels have 1024, 256, 64 and 16 rows per frame (side 64: four times as
many), so which levels run on the bf16 pipe and which fall to the fp32-MFMA kernels changes at F = 7, 13, 25, 50, 100, 200, 400 and
with F % 4 and F % 16.

`census(F, h)` is what decides the case table: the answers of the library's own dry-run routers (dawn_conv3x3_form,
dawn_conv3x3_direct_form, dawn_gemm1x1_form, and dawn_gemm1x1_ln_inline_ok / dawn_gemm1x1_split_ok wherever the orchestration asks them)
for every conv / GEMM call of one evaluation, in call order.  It drives the real orchestration (unet_forward.build_clip_state +
unet_forward) over `DryOps`, an op set that builds each call's descriptor with ops.conv_desc -- the function HipOps.conv_gemm builds
it with -- asks the routers and returns uninitialised tensors of the right shape: no arithmetic, no GPU.  CASES holds one case per
signature that occurs for F = 1..128 at h = 32 and F = 1..32 at h = 64 (test_length_gate_cpu.test_census_coverage); signatures that
first occur above those ranges are the existing T96 / C2 / C3 fixtures' (fullsize_cases.py), held at 1e-4 only.

NOT in the census: the temporal-attention and attention-core kernel selectors (dawn_temporal_layer_c64_ex, dawn_temporal_attn_ex,
the SLA / frame / cross-attention launches) have no dry-run query, so a signature says nothing about which of those kernels ran."""
import ctypes as C
import functools

import torch

from fullsize_cases import KW, build_inputs, checksum
import dawn_pytorch_amd as D
from dawn_pytorch_amd.ops import HipOps, conv_desc
from dawn_pytorch_amd.pack import pack_unet
from dawn_pytorch_amd.unet_forward import build_clip_state, unet_forward

WIN = KW["win_width"]

# (F, latent side h, diffusion time t).  The starting list, read from the thresholds above, was h = 32: F = 1, 3, 4, 6, 7, 13, 16, 25,
# 28, 50, 100, 112; h = 64: F = 1, 2, 4, 5, 7, 13, 25, 28.  The census found 21 signatures for F = 1..128 at h = 32 and 13 for
# F = 1..32 at h = 64; the cases of the second row of each side were added for the signatures the starting list missed (the lengths
# sharing each signature stand behind the case), and F = 13 at h = 32 left: its signature is that of F = 7 (the resample form counts
# output rows, so its 12800-row threshold lies at F = 50 there; F = 13 is a threshold at h = 64 only).  The times are arbitrary, spread
# over the schedule.
CASES = [
    (1, 32, 999), (3, 32, 12), (4, 32, 501), (6, 32, 850), (7, 32, 3), (16, 32, 700), (25, 32, 77), (28, 32, 940),
    (50, 32, 431), (100, 32, 166), (112, 32, 592),
    (8, 32, 219),        # 8, 24
    (10, 32, 655),       # 10, 14, 18, 22
    (12, 32, 38),        # 12, 20
    (26, 32, 806),       # 26, 30, .. 46
    (32, 32, 473),       # 32, 48
    (40, 32, 120),       # 40
    (51, 32, 911),       # every odd F from 51
    (52, 32, 564),       # 52, 60, .. 92
    (56, 32, 290),       # 56, 72, 88
    (96, 32, 627),       # 64, 80, 96: the clip of the reference fixture full_T96.npz (fullsize_cases.CASES["T96"]), which want64 is checked against
    (104, 32, 745),      # 104, 120
    (1, 64, 321), (2, 64, 888), (4, 64, 45), (5, 64, 777), (7, 64, 610), (13, 64, 129), (25, 64, 968), (28, 64, 364),
    (8, 64, 702),        # 8, 12
    (10, 64, 57),        # 10
    (14, 64, 836),       # 14, 18, 22
    (16, 64, 411),       # 16, 20, 24
    (26, 64, 193),       # 26, 30
]

# Cases that share a census signature, and what else distinguishes them (test_census_coverage allows exactly these):
SAME_SIGNATURE = {
    # a one-frame clip: the temporal layers attend over a single key, every per-frame table has one row, no frame boundary inside a tile
    ((1, 32), (3, 32)): "F = 1 is the one-frame clip",
}

# The gate factor of tests/test_hip_length_gates.py: rel_err(GPU, y64) <= C_LEN * e32 + split_gate.FLOOR.  By split_gate.py's rule: the
# largest ratio GPU error / e32 measured on an MI355X over all cases x 1.5, rounded up to the next 0.5.  Measured (all 35 cases in
# profiles/length_gate_ratios.md): 1.51 (F16_h32; 1.50 F1_h32 and F104_h32, 1.43 F96_h32, 0.82 the least, F28_h64) x 1.5 = 2.27 -> 2.5.
# A lost third weight plane on the census' split weights measures 5.27 / 5.61 x e32 on the two smallest cases
# (tests/test_length_gate_cpu.py): C_LEN is below 0.8 x that (4.2).
C_LEN = 2.5
C_CASE = {}                    # (F, h) -> a factor of its own, with its measurement stated beside it (none needed)

FIXTURE_LIMIT = 1 << 20        # bytes: no committed file is larger


def case_name(F, h):
    return f"F{F}_h{h}"


def fixture_name(F, h):
    return f"length_{case_name(F, h)}.npz"


def tail_frames(h):
    """Frames that share a 256-row tile with the ragged tail at the two deepest levels: rows per frame there are (h / 8)^2 and (h / 4)^2,
    so the deepest level's last tile spans 256 / (h / 8)^2 frames, and one more frame reaches the tile before it (h = 32: 17 frames)."""
    return 256 // (h // 8) ** 2 + 1


def kept_frames(F, h):
    """Every frame while y64 (3 x F x h x h float64) leaves the file under 1 MB; otherwise frame 0, every 8th frame and the last
    tail_frames(h) frames.  (h = 64: 5 tail frames, not the 17 of h = 32 -- 17 frames of 64 x 64 are 1.6 MB.)"""
    if 3 * F * h * h * 8 + 8192 < FIXTURE_LIMIT:
        return list(range(F))
    return sorted(set(range(0, F, 8)) | set(range(max(0, F - tail_frames(h)), F)))


# ---------------------------------------------------------------------------------------------- model and inputs
@functools.lru_cache(maxsize=1)
def full_unet():
    """The shipped architecture with seed-built weights (as tests/test_hip_fullsize.py) and their checksum."""
    unet = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    return unet, checksum(unet.state_dict().values())


def clip(F, h):
    """(x (1, 275, F, h, h), cond (1, F, 1032), inputs checksum): fullsize_cases.build_inputs, the frame-invariant channels expanded."""
    fea272, cond, x3 = build_inputs(F, h)
    return torch.cat((x3, fea272.unsqueeze(2).expand(-1, -1, F, -1, -1)), 1), cond, checksum([fea272, cond, x3])


def cast_sd(sd, dtype):
    return {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def oracle(sd, x, cond, t, dtype):
    """oracle.dawn_oracle.unet_forward in `dtype` -> (3, F, h, h).  float32 through torch's im2col + GEMM convolution (oneDNN and NNPACK
    off), as split_gate.Case.base32."""
    import warnings
    from oracle import dawn_oracle as O
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.backends.mkldnn.flags(enabled=False), torch.backends.nnpack.flags(enabled=False):
            return O.unet_forward(cast_sd(sd, dtype), x.to(dtype), torch.tensor([t]), cond.to(dtype), win=WIN, p="")[0]


# ---------------------------------------------------------------------------------------------- the census
class Census:
    """Mixin over HipOps: records the routers' answers (self.census, a list) where the orchestration asks them.  conv_gemm is recorded
    by the classes below (dry: from the descriptor; live: through form_only before the launch)."""

    def ln_inline_ok(self, rows, N, C0, C1=0):
        ok = super().ln_inline_ok(rows, N, C0, C1)
        self.census.append(("ln_inline_ok", N, C0 + C1, bool(ok)))
        return ok

    def split_gemm_ok(self, rows, N, C0, C1=0):
        ok = super().split_gemm_ok(rows, N, C0, C1)
        self.census.append(("split_ok", N, C0 + C1, bool(ok)))
        return ok

    def record_conv(self, KH, Hi, K, N, mode, form3, form1, direct):
        """One conv / GEMM call: its kind (kernel size, input height, K, N, mode -- none depends on F) and the three routers' answers."""
        self.census.append((f"conv{KH}" + ("T" if mode else ""), Hi, K, N, int(form3), int(form1), int(direct)))


class DryOps(Census, HipOps):
    """The op interface of HipOps without a launch: every op returns uninitialised tensors of the shapes (and aliasing) the real op
    returns, conv_gemm asks the routers about the descriptor HipOps.conv_gemm would launch.  Runs on CPU tensors."""

    def __init__(self):
        super().__init__()
        self.census = []
        self.split_w = set()         # id() of the weight of every call that a split-operand kernel takes (split_weights)

    def begin_evaluation(self, like):
        pass

    def fork_join(self, side, main):
        a = side()
        return a, main()

    def conv_gemm(self, in0, w, N, *, F, Hi, Wi, Ho=None, Wo=None, KH=1, KW=1, stride=1, pad=0, mode=0, out=None, gn_fin=None, **kw):
        Ho = Hi if Ho is None else Ho
        Wo = Wi if Wo is None else Wo
        if out is None:
            out = self.empty(F * Ho * Wo, N, like=in0)
        d = conv_desc(in0, w, N, out, F=F, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, KH=KH, KW=KW, stride=stride, pad=pad, mode=mode,
                      policy=self.conv_policy, sk_ws=self.sk_ws, **kw)
        forms = self.conv3x3_form(d), self.L.dawn_gemm1x1_form(C.byref(d)), self.L.dawn_conv3x3_direct_form(C.byref(d))
        self.record_conv(KH, Hi, d.C0 + d.C1, N, mode, *forms)
        if any(forms):
            self.split_w.add(id(w))
        return out

    def conv_gn_part(self, rows_out, N, like):
        return torch.empty(1, 16, dtype=torch.float64)

    def gn_coeffs(self, x, gamma, beta, film, total_rows, eps=1e-5, part=None):
        return self.empty(x.shape[1], like=x), self.empty(x.shape[1], like=x)

    def gn_apply_res(self, x, a, b, res, inplace=False):
        return x if inplace else self.empty(*x.shape, like=x)

    def ln_rowstats(self, in0, in1=None, eps=1e-5):
        return self.empty(in0.shape[0], like=in0), self.empty(in0.shape[0], like=in0)

    def ln_rows(self, in0, in1=None, eps=1e-5):
        return self.empty(in0.shape[0], in0.shape[1] + (0 if in1 is None else in1.shape[1]), like=in0)

    def xattn_prep(self, kv, k_scale, null_kv, kvtab, branch, nulltab):
        pass

    def xattn_core(self, q, HW, kvtab, nulltab, q_scale):
        return q

    def xattn_ln_sum(self, y3, g3, Co, eps=1e-5):
        return self.empty(y3.shape[0], Co, like=y3)

    def xattn_tables(self, kvtab, nulltab, q_scale, wo, Co):
        return self.empty(kvtab.shape[0], 3, 64 + 9 * Co, like=kvtab)

    def xattn_sigma_out(self, q, HW, xtab, g3, Co, eps=1e-5, gn=None, h1_over_c1=False):
        return gn[0] if (h1_over_c1 and gn is not None) else self.empty(q.shape[0], Co, like=q)

    def xattn_layer_c64(self, x, x2, HW, wq, wo, g3, q_scale, kvtab, nulltab, eps=1e-5, xtab=None, wq_bf3=None, gn=None, h1_over_c1=False):
        return gn[0] if (h1_over_c1 and gn is not None) else self.empty(x.shape[0], 64, like=x)

    def temporal_attn(self, qkv, Fext, HW, q0, Fq, win, rcos, rsin, band):
        return self.empty(Fq * HW, 256, like=qkv)

    def temporal_layer_c64(self, x, Fext, HW, q0, Fq, win, wqkv, wout, rcos, rsin, band, eps=1e-5, wqkv_bf3=None, wout_bf3p=None, out=None):
        return self.empty(Fq * HW, 64, like=x) if out is None else out

    def sla(self, qkv, F, HW):
        return self.empty(F * HW, 256, like=qkv)

    def sla_layer_c64(self, x, F, HW, wqkv, wout, bias, eps=1e-5, wqkv_bf3=None, out=None):
        return self.empty(F * HW, 64, like=x) if out is None else out

    def frame_attn(self, qkv, F, N):
        return self.empty(F * N, 256, like=qkv)

    def init_conv_x(self, x, w3, fea_pre, F, h, w, Co, frames=None, out=None):
        fa, fb = frames if frames is not None else (0, F)
        return self.empty((fb - fa) * h * w, Co, like=x) if out is None else out

    def head_out(self, hg, ho, wg, bg, wo, bo, out=None):
        ref = hg if hg is not None else ho
        return self.empty(3, ref.shape[0], like=ref) if out is None else out

    def heads_eps(self, gn_g, gn_o, x, x2, wg, wo, wf, bf, out=None):
        return self.empty(3, x.shape[0], like=x) if out is None else out

    def linear(self, x, W, bias, act_in=0, out=None):
        return self.empty(x.shape[0], W.shape[0], like=x) if out is None else out

    def sinusoidal(self, t, freqs):
        return self.empty(1, 2 * freqs.numel(), like=freqs)


@functools.lru_cache(maxsize=1)
def packed_cpu():
    return pack_unet(dict(full_unet()[0].state_dict()), WIN, "cpu", prefix="")


@functools.lru_cache(maxsize=None)
def census(F, h):
    """The signature of one evaluation (clip state + forward) of an F-frame clip at latent side h: a tuple, see the module docstring."""
    ops, P = DryOps(), packed_cpu()
    cs = build_clip_state(ops, P, torch.empty(272, h, h), torch.empty(F, KW["cond_dim"]), WIN)
    unet_forward(ops, P, cs, torch.empty(3, F, h, h), 0)
    return tuple(ops.census)


def packed_weight_names(P):
    """id(packed weight tensor that conv_gemm is called with) -> the state-dict keys it was packed from."""
    from dawn_pytorch_amd.pack import BRANCHES
    m = {}

    def rb(r, p):
        m[id(r.w1)], m[id(r.w2)] = [p + "block1.proj.weight"], [p + "block2.proj.weight"]
        if r.wr is not None:
            m[id(r.wr)] = [p + "res_conv.weight"]
        if r.conditioned:
            m[id(r.wq)] = [p + f"cross_attn_{br}.to_q.weight" for br in BRANCHES]
            for b, br in enumerate(BRANCHES):
                m[id(r.wo[b])] = [p + f"cross_attn_{br}.to_out.0.weight"]

    def attn(a, p, inner="fn.fn.fn."):
        m[id(a.wqkv)], m[id(a.wout)] = [p + inner + "to_qkv.weight"], [p + inner + "to_out.weight"]

    attn(P.init_tattn, "init_temporal_attn.")
    for side, lvls in (("downs", P.downs), ("ups", P.ups)):
        for l, lvl in enumerate(lvls):
            q = f"{side}.{l}."
            rb(lvl["rb1"], q + "0.")
            rb(lvl["rb2"], q + "1.")
            attn(lvl["sla"], q + "2.", "fn.fn.")
            attn(lvl["tattn"], q + "3.")
            rs = lvl.get("down") or lvl.get("up")
            if rs is not None:
                m[id(rs[0])] = [q + "4.weight"]
    rb(P.mid["rb1"], "mid_block1.")
    rb(P.mid["rb2"], "mid_block2.")
    attn(P.mid["sattn"], "mid_spatial_attn.")
    attn(P.mid["tattn"], "mid_temporal_attn.")
    rb(P.head_g, "final_conv.0.")
    rb(P.head_o, "occlusion_map.0.")
    return m


def split_weights(F, h):
    """The state-dict keys of every weight that the census of (F, h) sends to a split-operand kernel: the weight of each conv_gemm call
    whose descriptor a Winograd form, a direct split 3x3 form or a split 1x1 / resample form takes.  (The fused 64-channel attention
    layers split their weights too; they are no conv_gemm calls and not in the census.)"""
    ops, P = DryOps(), packed_cpu()
    cs = build_clip_state(ops, P, torch.empty(272, h, h), torch.empty(F, KW["cond_dim"]), WIN)
    unet_forward(ops, P, cs, torch.empty(3, F, h, h), 0)
    names = packed_weight_names(P)
    return sorted(k for i in ops.split_w for k in names[i])


def signature_digest(sig):
    """A short stable name of a signature (for logs and the ratio table)."""
    import hashlib
    return hashlib.sha1(repr(sig).encode()).hexdigest()[:10]
