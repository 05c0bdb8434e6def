"""The fp32-accuracy gate of tests/split_gate.py on the kernels of the two stages around the UNet: the HuBERT audio-feature stage
(csrc/hubert.hip, hubert.py; its conv layers and Linears are 1-D problems on the generic fp32-MFMA implicit GEMM of dawn_conv_gemm) and
the PBnet pose / blink stage (csrc/pbnet.hip, pbnet.py, dawn_linear).  The gate, its factor and its floor are split_gate's:

    rel_err(got) <= c * rel_err(base32) + FLOOR,      rel_err(t) = max|t - want64| / max|want64|,      c = C_GATE unless the case widens it,

want64 = the RefOps op of the case in float64 on the CPU, base32 = the same op in float32 on the CPU (convolutions through torch's
im2col + GEMM, for the reason split_gate's docstring gives; wave_normalize through numpy's own float32 mean / var, the reference's
arithmetic).  tests/test_stage_gate_cpu.py shows on the CPU that every case accepts base32 and rejects the defects of `Case.defects`, each
emulated in float64 against the same want64 and checked with the case's own c; tests/test_hip_stage_fp64_gates.py runs the same cases
on the GPU kernels.

Shapes: channel counts and tap geometry are those of hubert-large (7 x 512 conv stack, 1024 wide, 16 heads of 64, FFN 4096, 128-tap / 16-group
positional conv) and of the shipped PBnet decoders (d 64, 4 heads of 32, ff 1024, audio 1024, latent 256), because they fix the kernel
instantiation; only the number of frames T is reduced.

The defects.
  precision   one matrix operand truncated to its top 16 mantissa bits (`trunc16`: the first two planes of split_gate.trunc_planes3), what
              a tf32-class matrix pipe would compute.  Convolutions and Linears: the weights, which `coherent` draws so that the lost bits
              are as large as they can be and carry the weight's sign; attn64 / attn_bias32: Q and K where the kernels form the score
              product (after the scale and the rotary).  With ONE key (attn64 at T = 1) the softmax is 1 whatever the scores are and Q and K
              do not reach the output: there the defect is applied to V, the only operand that does.
  structure   convs: the last K chunk lost (the last BK = 16 or 32 input channels of the last tap); the last output row taken from a window
              shifted by one input sample (what lies behind the input reads as zero).  Positional conv: the neighbouring group's columns read.
              attn64: `alpha` omitted from the running O and l -- invisible in every regime at T <= 32, which is ONE 32-key tile (alpha
              multiplies an empty O and l there), so those T are exempt from this defect only; and the keys after the last full 32-key
              tile lost -- there are none where T % 32 == 0, and with T < 32 no key would be left at all: T in {33, 65, 999, 1000} carry it.
LayerNorm, wave_normalize, add_act carry no emulated defect: their cases check that CPU fp32 has a real fp32 error against float64 on
this data, so that the GPU kernel is held to fp32 accuracy where it is hard (outlier channels, a DC offset 30 x the signal, GELU's tails).

attn_bias32: every query row keeps at least its diagonal key unmasked.  In a fully masked row fp32 absorbs the scores into -1e8 (all
keys equal: a uniform softmax) and float64 does not (the scores still order the keys), so the two references disagree by construction."""
import warnings

import numpy as np
import torch

from oracle.ops_ref import RefOps
from split_gate import C_GATE, FLOOR, LOG, coherent, fp32_gate, gate_rejects, packd, rel_err, trunc_planes3  # noqa: F401 (re-exported)

SENTINEL = 1234.5          # what the positional conv's output buffer holds outside the group's columns
HEADS64, HEADS32 = 16, 4

# Gate factors widened past C_GATE: GPU error / CPU fp32 error against float64 measured on an MI355X (max over that kernel's cases), x 1.5,
# rounded up to the next 0.5 (the rule of split_gate.C_TILED ...).  Kernels that are not named here hold C_GATE = 2; their measured maxima:
# attn64 1.51 (a), 1.03 (b), 1.01 (c); ln_affine_act 1.31; hubert_conv0 1.00; wave_normalize 0.84; add_act 1.00; attn_bias32 1.57; linear 1.08.
C_WIDE = {
    # conv_gemm_glds_kernel (the generic fp32-MFMA implicit GEMM, direct-to-LDS staging) with its two-level K accumulation: 2.32 (FFN up,
    # K = 1024; 2.27 / 2.16 on the feature-extractor convs, 1.81 at K = 4096, 1.60 at K = 8192).  Before the accumulators were folded every
    # 512 products the one fp32 chain over K measured 6.42 (K = 1536), 9.30 (K = 4096) and 11.96 (K = 8192): factors of 10 / 14 / 18, at
    # which test_stage_gate_cpu no longer rejects the tf32-class operand at K = 8192 (its error is 18.3x CPU fp32's there).
    "hconv": 3.5,
}


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def trunc16(x):
    """x (float32 values) with every element truncated to its top 16 mantissa bits, as float64."""
    p1, p2, _ = trunc_planes3(x.float())
    return p1.double() + p2.double()


def _cpu_fp32(fn):
    """fn() with torch's im2col + GEMM convolution (oneDNN and NNPACK off), as split_gate.Case.base32."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.backends.mkldnn.flags(enabled=False), torch.backends.nnpack.flags(enabled=False):
            return fn()


# ---------------------------------------------------------------------------------------------- hooked float64 references
# RefOps.attn64 / RefOps.attn_bias32 in float64 with a hook where the kernels form the score product.  Without hooks they are the RefOps
# ops (test_stage_gate_cpu.test_hooked_reference_is_the_oracle).
def attn64_64(qkv, heads, qk=None, v_fn=None, no_alpha=False, lose_tail=False):
    """qk: applied to the scaled Q and to K before S = Q K^T; v_fn: to V.  no_alpha: the online softmax of attn64_kernel over 32-key tiles
    with the rescale of the running O and l left out.  lose_tail: the keys after the last full 32-key tile never reach the softmax."""
    T = qkv.shape[0]
    q, k, v = (t.reshape(T, heads, 64).transpose(0, 1) for t in qkv.double().chunk(3, dim=1))
    q = q * 0.125
    if qk is not None:
        q, k = qk(q), qk(k)
    if v_fn is not None:
        v = v_fn(v)
    s = q @ k.transpose(1, 2)
    if lose_tail:
        Tt = (T // 32) * 32
        s, v = s[:, :, :Tt], v[:, :Tt]
    if no_alpha:
        m = torch.full((heads, T, 1), -3.0e38, dtype=torch.float64)
        l = torch.zeros(heads, T, 1, dtype=torch.float64)
        o = torch.zeros(heads, T, 64, dtype=torch.float64)
        for j0 in range(0, s.shape[2], 32):
            st = s[:, :, j0:j0 + 32]
            m = torch.maximum(m, st.amax(-1, keepdim=True))
            p = (st - m).exp()
            l, o = l + p.sum(-1, keepdim=True), o + p @ v[:, j0:j0 + 32]
        o = o / l
    else:
        o = torch.softmax(s, dim=-1) @ v
    return o.transpose(0, 1).reshape(T, heads * 64).contiguous()


def attn32_64(q, k, v, heads, bias, rcos, rsin, scale, qk=None):
    """RefOps.attn_bias32 in float64; qk: applied to the scaled, rotated Q and to the rotated K (what attn_bias32_kernel multiplies)."""
    q, k, v, bias, rcos, rsin = (t.double() for t in (q, k, v, bias, rcos, rsin))

    def split(t):
        return t.reshape(t.shape[0], heads, 32).transpose(0, 1)

    def rot(t):
        n, nr = t.shape[1], rcos.shape[1]
        c, s = rcos[:n].repeat_interleave(2, dim=1), rsin[:n].repeat_interleave(2, dim=1)
        tr, tp = t[..., :2 * nr], t[..., 2 * nr:]
        x = tr.reshape(*tr.shape[:-1], nr, 2)
        half = torch.stack((-x[..., 1], x[..., 0]), dim=-1).reshape(tr.shape)
        return torch.cat((tr * c + half * s, tp), dim=-1)
    qh, kh, vh = rot(split(q) * scale), rot(split(k)), split(v)
    if qk is not None:
        qh, kh = qk(qh), qk(kh)
    sim = qh @ kh.transpose(1, 2) + bias
    sim = sim - sim.amax(dim=-1, keepdim=True)
    return (sim.softmax(dim=-1) @ vh).transpose(0, 1).reshape(q.shape[0], heads * 32).contiguous()


# ---------------------------------------------------------------------------------------------- cases
class Case:
    """name, kind, parameters.  make() -> the seeded float32 inputs; want64 / base32 -> the two references; defects() -> {name: result of
    the defective op in float64}."""

    def __init__(self, name, kind, c=None, **p):
        self.name, self.kind, self.p = name, kind, p
        self.c = C_WIDE.get(kind, C_GATE) if c is None else c

    def __repr__(self):
        return self.name

    # ------------------------------------------------------------------ inputs
    def make(self):
        p, k = self.p, self.kind
        if k == "hconv":
            C0, N, KW = p["C0"], p["N"], p.get("KW", 1)
            Wi, Wo = self.rows_in(), self.rows_out()
            K = KW * C0
            g = p.get("group")
            buf = rnd(Wi, C0 if g is None else 1024, seed=1)           # (pos conv: the other groups' columns hold other random data)
            return dict(buf=buf, w=coherent(rnd(K, N, seed=2, scale=K ** -0.5)), bias=rnd(N, seed=3),
                        res=rnd(Wo, N, seed=4) if p.get("res") else None)
        if k == "attn64":
            T, reg = p["T"], p["regime"]
            qkv = rnd(T, 3 * HEADS64 * 64, seed=T, scale=1.2 if reg == "a" else 3.0)
            if reg == "c":       # keys drift along a unit vector per head that every query leans on: the running maximum keeps rising along T
                u = rnd(HEADS64, 64, seed=9)
                u = u / u.norm(dim=1, keepdim=True)
                x = qkv.view(T, 3, HEADS64, 64)
                x[:, 1] += (torch.arange(T).float()[:, None, None] / T * 12.0) * u
                x[:, 0] += 6.0 * u
            return dict(qkv=qkv)
        if k == "ln":
            rows, C = p["rows"], p["C"]
            x = rnd(rows, C, seed=1) + rnd(rows, 1, seed=2, scale=3.0)            # per-row offset
            for ch, v in ((7, 300.0), (C // 2 + 1, -300.0), (C - 3, 300.0)):         # three outlier channels
                x[:, ch] += v
            return dict(x=x, g=rnd(C, seed=3) * 0.3 + 1, b=rnd(C, seed=4) * 0.2)
        if k == "conv0":
            return dict(x=rnd(p["n"], seed=1), w=coherent(rnd(512, 10, seed=2, scale=0.3)), bias=rnd(512, seed=3, scale=0.1))
        if k == "wavenorm":
            return dict(x=rnd(p["n"], seed=1) * 0.003 + 0.1)                         # a quiet recording with a DC offset
        if k == "addact":
            b = torch.cat((torch.linspace(-30.0, 30.0, 128 * 33), rnd(128 * 300, seed=1, scale=8.0).clamp(-30, 30))).reshape(333, 128)
            return dict(a=None if p.get("inplace") else rnd(333, 128, seed=2), b=b)
        if k == "attn32":
            Tq, Tk, hd = p["Tq"], p["Tk"], HEADS32 * 32
            n = max(Tq, Tk)
            rel = torch.arange(Tk)[None, :] - torch.arange(Tq)[:, None]
            bias = rnd(HEADS32, Tq, Tk, seed=4, scale=1.5) - 1e8 * (rel.abs() > 100).float()      # eval-mode window: the diagonal stays
            ang = torch.arange(n).float()[:, None] * (1.0 / 10000 ** (torch.arange(2).float() / 2))[None]
            return dict(qkv=rnd(n, 3 * hd, seed=1, scale=p["sigma"]), bias=bias, rc=ang.cos().contiguous(), rs=ang.sin().contiguous())
        if k == "linear":
            K, N = p["K"], p["N"]
            return dict(x=rnd(200, K, seed=1), W=coherent(rnd(N, K, seed=2, scale=1.2 * K ** -0.5)), bias=rnd(N, seed=3, scale=0.2))
        raise ValueError(k)

    # ------------------------------------------------------------------ geometry of the hubert conv_gemm launches
    def rows_in(self):
        p = self.p
        return p["T"] + (128 if p.get("group") is not None else 0)                   # the positional conv reads the padded buffer

    def rows_out(self):
        p = self.p
        return p["T"] if p.get("group") is not None else (p["T"] - p.get("KW", 1)) // p.get("stride", 1) + 1

    def conv_kw(self):
        """The keyword set HubertFeatures.encode passes for this launch (without bias / res / out)."""
        p = self.p
        if p.get("KW", 1) == 1:
            return dict(F=1, Hi=1, Wi=p["T"])
        return dict(F=1, Hi=1, Wi=self.rows_in(), Ho=1, Wo=self.rows_out(), KH=1, KW=p["KW"], stride=p.get("stride", 1), pad=0)

    def x_of(self, T_, group=None):
        g = self.p.get("group") if group is None else group
        return T_["buf"] if g is None else T_["buf"][:, g * 64:(g + 1) * 64]

    # ------------------------------------------------------------------ the op
    def ref(self, T_, dtype, **over):
        """The RefOps op on the inputs cast to dtype; `over` replaces inputs (already in dtype)."""
        ops = RefOps()
        k, p = self.kind, self.p
        t = {n: (over[n] if n in over else (v.to(dtype) if torch.is_tensor(v) else v)) for n, v in T_.items()}
        if k == "hconv":
            x = over["x"] if "x" in over else self.x_of(T_).to(dtype)
            return ops.conv_gemm(x, packd(t["w"]), p["N"], bias=t["bias"], res=t["res"], **self.conv_kw())
        if k == "attn64":
            return ops.attn64(t["qkv"], HEADS64)
        if k == "ln":
            return ops.ln_affine_act(t["x"], t["g"], t["b"], 1e-5, p["act"])
        if k == "conv0":
            return ops.hubert_conv0(t["x"], t["w"], t["bias"], 5)
        if k == "addact":
            return ops.add_act(t["a"], t["b"], 2)
        if k == "attn32":
            q, k_, v = self.qkv32(t["qkv"])
            return ops.attn_bias32(q, k_, v, HEADS32, t["bias"], t["rc"], t["rs"], 32 ** -0.5)
        if k == "linear":
            return ops.linear(t["x"], t["W"], t["bias"], act_in=p["act_in"])
        raise ValueError(k)

    def qkv32(self, qkv):
        """Strided q | k | v views of one buffer, as PoseBlinkGenerator._self_attn slices its to_qkv output."""
        hd = HEADS32 * 32
        return qkv[:self.p["Tq"], :hd], qkv[:self.p["Tk"], hd:2 * hd], qkv[:self.p["Tk"], 2 * hd:]

    def want64(self, T_):
        if self.kind == "wavenorm":
            x = T_["x"].numpy().astype(np.float64)
            return torch.from_numpy((x - x.mean()) / np.sqrt(x.var() + 1e-7))
        return self.ref(T_, torch.float64)

    def base32(self, T_):
        if self.kind == "wavenorm":                 # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm on a float32 array
            x = T_["x"].numpy()
            return torch.from_numpy((x - x.mean()) / np.sqrt(x.var() + 1e-7))
        return _cpu_fp32(lambda: self.ref(T_, torch.float32))

    # ------------------------------------------------------------------ the defects (see the module docstring)
    def defect_names(self):
        k, p = self.kind, self.p
        if k == "hconv":
            return ("precision", "last_chunk_lost", "last_row_shifted") + (("neighbour_group",) if p.get("group") is not None else ())
        if k == "attn64":
            T = p["T"]
            return ("precision",) + (("no_alpha",) if T > 32 else ()) + (("tail_keys_lost",) if T > 32 and T % 32 else ())
        if k == "conv0":
            return ("precision", "last_row_shifted")
        if k in ("attn32", "linear"):
            return ("precision",)
        return ()

    def defects(self, T_, want64):
        k, p = self.kind, self.p
        out = {}
        if k == "hconv":
            w = T_["w"]
            out["precision"] = self.ref(T_, torch.float64, w=trunc16(w))
            lost = w.double().clone()
            lost[-p["bk"]:] = 0
            out["last_chunk_lost"] = self.ref(T_, torch.float64, w=lost)
            # the last row from the window one input sample further on (zero behind the input)
            x = torch.cat((self.x_of(T_).double(), torch.zeros(1, p["C0"], dtype=torch.float64)))
            KW, st, last = p.get("KW", 1), p.get("stride", 1), self.rows_out() - 1
            row = x[last * st + 1:last * st + 1 + KW].reshape(-1) @ w.double() + T_["bias"].double()
            if T_["res"] is not None:
                row = row + T_["res"][last].double()
            out["last_row_shifted"] = want64.clone()
            out["last_row_shifted"][last] = row
            if p.get("group") is not None:
                g = p["group"]
                out["neighbour_group"] = self.ref(T_, torch.float64, x=self.x_of(T_, g + 1 if g == 0 else g - 1).double())
        elif k == "attn64":
            qkv, T = T_["qkv"], p["T"]
            if T == 1:
                out["precision"] = attn64_64(qkv, HEADS64, v_fn=trunc16)
            else:
                out["precision"] = attn64_64(qkv, HEADS64, qk=trunc16)
            if "no_alpha" in self.defect_names():
                out["no_alpha"] = attn64_64(qkv, HEADS64, no_alpha=True)
            if "tail_keys_lost" in self.defect_names():
                out["tail_keys_lost"] = attn64_64(qkv, HEADS64, lose_tail=True)
        elif k == "conv0":
            out["precision"] = self.ref(T_, torch.float64, w=trunc16(T_["w"]))
            x = torch.cat((T_["x"].double(), torch.zeros(1, dtype=torch.float64)))
            last = want64.shape[0] - 1
            out["last_row_shifted"] = want64.clone()
            out["last_row_shifted"][last] = T_["w"].double() @ x[last * 5 + 1:last * 5 + 11] + T_["bias"].double()
        elif k == "attn32":
            q, k_, v = self.qkv32(T_["qkv"])
            out["precision"] = attn32_64(q, k_, v, HEADS32, T_["bias"], T_["rc"], T_["rs"], 32 ** -0.5, qk=trunc16)
        elif k == "linear":
            out["precision"] = self.ref(T_, torch.float64, W=trunc16(T_["W"]))
        assert tuple(out) == self.defect_names(), (self.name, tuple(out))
        return out


def _hconv(name, **p):
    # BK of the generic kernel's K loop: 32 where K >= 2304 and N >= 256 (conv_gemm.hip `deep`, and ConvPolicy.BK32 at K >= 4096), else 16
    K = p.get("KW", 1) * p["C0"]
    return Case(f"hubert_conv/{name}", "hconv", bk=32 if K >= 2304 and p["N"] >= 256 else 16, **p)


ATTN64_T = (1, 31, 32, 33, 64, 65, 999, 1000)           # both sides of the 32-key and 32-query tile edges, and the full 20 s chunk
ATTN32_SHAPES = ((200, 200), (1, 5), (65, 64), (64, 65), (70, 201))

CASES = [
    # ---- HuBERT conv_gemm launches (F = 1, Hi = Ho = 1, KH = 1, bias: the keyword sets of HubertFeatures.encode)
    _hconv("fe_k3s2_T320", C0=512, N=512, KW=3, stride=2, T=320),               # To = 159 = 128 + 31 rows, one left-over sample
    _hconv("fe_k2s2_T79", C0=512, N=512, KW=2, stride=2, T=79),                 # To = 39: less than one tile, odd T
    _hconv("proj_512_1024_M49", C0=512, N=1024, T=49),
    # one group of the positional conv: a column slice of the (T + 128, 1024) buffer in, a column slice of a (T, 1024) buffer out
    _hconv("pos_g0_T150", C0=64, N=64, KW=128, T=150, group=0),
    _hconv("pos_g15_T150", C0=64, N=64, KW=128, T=150, group=15),
    _hconv("qkv_1024_3072_T150", C0=1024, N=3072, T=150),
    _hconv("out_1024_1024_res_T150", C0=1024, N=1024, T=150, res=True),
    _hconv("ffn_up_1024_4096_T150", C0=1024, N=4096, T=150),
    _hconv("ffn_down_4096_1024_res_T150", C0=4096, N=1024, T=150, res=True),
    _hconv("qkv_1024_3072_T1", C0=1024, N=3072, T=1),
    # ---- attn64: (a) unit scale, (b) score std ~ 9, (c) = (b) with a drift that keeps raising the running maximum along the keys
    *[Case(f"attn64/T{T}_{reg}", "attn64", T=T, regime=reg) for reg in "abc" for T in ATTN64_T],
    # ---- the two-pass LayerNorm of hubert.hip on a stable-layer-norm residual stream: outlier channels at +-300, a per-row offset;
    # rows 1 and 5: a partial last workgroup (4 rows each)
    *[Case(f"ln_affine_act/r{rows}_C{C}_act{act}", "ln", rows=rows, C=C, act=act) for C in (512, 1024, 4096) for act in (0, 2)
      for rows in (1, 5, 64)],
    # ---- the Cin = 1 first conv: (n - 10) % 5 = 0 (no sample left over) and 4
    Case("hubert_conv0/n4010", "conv0", n=4010),
    Case("hubert_conv0/n4014", "conv0", n=4014),
    Case("wave_normalize/quiet_dc_n48077", "wavenorm", n=48077),
    Case("add_act/gelu_pm30", "addact"),
    Case("add_act/gelu_pm30_inplace", "addact", inplace=True),
    # ---- PBnet: attn_bias32 (4 heads, 2 rotary pairs, window mask) at unit scale and at score std ~ 9; dawn_linear at the decoder's shapes
    *[Case(f"attn_bias32/{Tq}x{Tk}_sigma{sg}", "attn32", Tq=Tq, Tk=Tk, sigma=sg) for sg in (1, 3) for Tq, Tk in ATTN32_SHAPES],
    *[Case(f"linear/K{K}_N{N}_act{a}", "linear", K=K, N=N, act_in=a) for K, N in ((1024, 256), (576, 64), (64, 1024), (1024, 64), (64, 6))
      for a in (0, 1)],
]
