"""The fp32-accuracy gate of the split-bf16 kernels, and the cases it runs on.

Every matrix kernel on the hot path splits its fp32 operands exactly into three bf16 planes and sums six cross terms in fp32, so its error
against a float64 evaluation of the same op must be that of an fp32 computation.  `fp32_gate` asserts

    rel_err(got) <= C_GATE * rel_err(base32) + FLOOR,      rel_err(t) = max|t - want64| / max|want64|,

where want64 is the RefOps op (oracle/ops_ref.py) evaluated in float64 on CPU and base32 the same op in float32 on CPU (`Case.base32`:
with torch's im2col + GEMM convolution -- oneDNN's direct convolution sums K almost in sequence and NNPACK transforms in fp32: at
K >= 1152 their own error of 1..15e-6 is as large as the defects below).  Comparing with CPU fp32 at 1e-4 cannot see a kernel that has
lost its third weight plane; this gate can, and tests/test_split_gate_cpu.py proves it for every case below: it rejects the two plane
defects emulated in torch (`drop_third`, `stale_third`) and accepts the fp32 CPU result.  tests/test_hip_fp64_gates.py runs the same
cases on the GPU kernels.

The attention kernels also split ACTIVATIONS in the kernel (ACT_OPERANDS: X, Q, K, V, P, O): the hooked float64 references below
(`attn_core64`, `temporal_layer64`) apply a defect to one such operand where the kernels split it, and the CPU test shows that the gate
rejects each operand's third plane dropped (`drop_third_act`) or read from the previous head (`stale_third_act`).  The fp32 attention
kernels (temporal_attn_kernel, SLA, frame attention, the unfused cross-attention chain) are held to the same gate.

The split weights are drawn by `coherent` (except where the op normalises them away, see xattn): random magnitudes and signs, with the low bits set so that the third bf16 plane is as large
as it can be and has the weight's sign.  A lost or stale third plane then moves every output by ~7e-6 of its size, whatever K is --
with independent random low bits the defect averages out to 2..3e-6, no larger than the GPU kernels' own fp32 accumulation error at
K >= 512 (measured up to 6x CPU fp32 GEMM's), and no single gate factor could tell them apart.

C_GATE is 2, as for the shipped direct 3x3 gate.  Where the MI355X measurement needs more, the case carries its own `c`, and the
measured ratio (GPU error / CPU fp32 error, max over the cases of that kernel) is stated beside it.

A case is (name, kind, params).  Shapes are production ones (profiles/r6_insitu_shapes.txt = configs[2],
profiles/r6_config1_insitu_shapes.txt = configs[1]): H, W and the channel counts, which fix the kernel instantiation and tile geometry, are
kept; only the number of frames (rows) is reduced.  `split` names the weights the kernel consumes as bf16 planes: the mutants change only
those.  `form` is what dawn_conv3x3_form / dawn_gemm1x1_form must answer for the case's descriptor and `direct`, where given, the answers
dawn_conv3x3_direct_form may give: both are asserted before the launch."""
import json
import math
import os
import warnings

import torch

from dawn_pytorch_amd.policy import ConvPolicy
from test_hip_ops import LOG      # the op-error log every GPU op test appends to (test_hip_ops.check)

C_GATE = 2.0          # the factor of the whole file; a case widens it only with a measured reason stated beside it
FLOOR = 1e-7          # relative to max|want64|: ~1 ulp of fp32 at the output's scale
DEFAULT_POLICY = ConvPolicy.DEFAULT
TILED_ONLY = ConvPolicy.TILED_ONLY        # DEFAULT | NO_ROW_KERNELS: the tiled split kernel for every 1x1 shape (reaches its nS = 2 corner)


# ---------------------------------------------------------------------------------------------- the gate
def rel_err(t, want64):
    return float((t.detach().cpu().double() - want64).abs().max() / want64.abs().max())


def fp32_gate(name, got, want64, base32, c=C_GATE, floor=FLOOR, log=True):
    """Assert that `got` is as accurate as CPU fp32 (see the module docstring); append its errors to the op-error log (LOG)."""
    return fp32_gate_e32(name, got, want64, rel_err(base32, want64), c, floor, log)


def fp32_gate_e32(name, got, want64, e32, c=C_GATE, floor=FLOOR, log=True, **extra):
    """fp32_gate where CPU fp32's own error e32 = rel_err(base32, want64) was measured beforehand (the fixtures of length_cases.py hold
    it beside want64); `extra` goes into the record."""
    got = got.detach().cpu().double()
    diff = got - want64
    e = rel_err(got, want64)
    rec = {"op": f"fp64_gate/{name}", "rel_err": e, "rel_err_cpu_fp32": e32, "ratio": e / e32 if e32 > 0 else float("inf"),
           "max_abs_err": float(diff.abs().max()), "rms_err": float(diff.pow(2).mean().sqrt()), "scale": float(want64.abs().max()),
           "c": c, "floor": floor, "nan": bool(torch.isnan(got).any()), **extra}
    if log:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    assert not rec["nan"], f"{name}: NaN"
    assert e <= c * e32 + floor, f"{name}: rel err {e:.3e} > {c} x fp32's {e32:.3e} + {floor:.0e} (ratio {rec['ratio']:.2f})"
    return rec


def gate_rejects(got, want64, base32, c=C_GATE, floor=FLOOR):
    return rel_err(got, want64) > c * rel_err(base32, want64) + floor


# ---------------------------------------------------------------------------------------------- the plane defects
def planes3(w):
    """The exact split w = w1 + w2 + w3 of dawn_pytorch_amd.pack.pack_bf3, as float32 tensors.
    In the kernels: dawn_split3_rne_quad (csrc/dawn_common.h), round to nearest even."""
    w = w.float()
    w1 = w.to(torch.bfloat16).float()
    r1 = w - w1
    w2 = r1.to(torch.bfloat16).float()
    return w1, w2, (r1 - w2).to(torch.bfloat16).float()


def drop_third(w):
    """Every weight truncated to its top two planes (the a1 . b3 term lost)."""
    w1, w2, _ = planes3(w)
    return w1.double() + w2.double()


def stale_third(w, seed=1234):
    """The third plane taken from another matrix of the same statistics (a prefetch of the wrong head / stage)."""
    g = torch.Generator().manual_seed(seed)
    other = torch.randn(w.shape, generator=g) * float(w.float().std())
    w1, w2, _ = planes3(w)
    return w1.double() + w2.double() + planes3(other)[2].double()


def trunc_planes3(x):
    """The exact split of dawn_split3_oct (csrc/dawn_common.h), the in-kernel split of every activation operand but X: p1 = the top 16
    bits of x, p2 = the top 16 bits of x - p1, p3 = the top 16 bits of what is left (all fp32 subtractions, exact).  Float32 tensors."""
    hi = lambda t: (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    x = x.float()
    p1 = hi(x)
    r = x - p1
    p2 = hi(r)
    return p1, p2, hi(r - p2)


def drop_third_act(t, split, axis):
    """The operand t (float64) as the kernel would use it with the third plane of its fp32 value lost (the a3 terms dropped)."""
    return t - split(t.float())[2].double()


def stale_third_act(t, split, axis):
    """... with the third plane read from the neighbour along `axis`: the same operand of the previous head (the K / V planes are
    rewritten by every head behind one barrier: a race on it reads the previous head's), for X the previous frame row."""
    p3 = split(t.float())[2].double()
    return t - p3 + p3.roll(1, dims=axis)


ACT_DEFECTS = (drop_third_act, stale_third_act)


# ---------------------------------------------------------------------------------------------- hooked fp64 references
# RefOps.temporal_attn and RefOps.temporal_layer_c64 (oracle/ops_ref.py) in float64, with a hook on every operand the kernels split in
# the kernel: `defect = {operand: fn}`, fn(t, split, axis) as drop_third_act.  Each hook sits where the kernels split that operand.
# Without hooks these are the RefOps ops (test_split_gate_cpu.test_hooked_reference_is_the_oracle).
LOG2E = math.log2(math.e)


def _hook(defect, name, t, split, axis):
    fn = (defect or {}).get(name)
    return t if fn is None else fn(t, split, axis)


def attn_core64(qkv, Fext, HW, q0, Fq, win, rcos, rsin, band, defect=None):
    """RefOps.temporal_attn in float64 with hooks on Q, K, V and P (all split by dawn_split3_oct / dawn_split3_trunc_quad: trunc_planes3)."""
    x = qkv.double().reshape(Fext, HW, 3, 8, 32)
    rcos, rsin, band = rcos.double(), rsin.double(), band.double()
    q = x[:, :, 0].permute(1, 2, 0, 3) * 32 ** -0.5          # (HW, 8, Fext, 32): axis 1 = head
    k = x[:, :, 1].permute(1, 2, 0, 3)
    v = x[:, :, 2].permute(1, 2, 0, 3)

    def rot(t):
        c, s = rcos[:Fext], rsin[:Fext]
        t1, t2 = t[..., 0::2], t[..., 1::2]
        return torch.stack((t1 * c - t2 * s, t2 * c + t1 * s), dim=-1).flatten(-2)

    q, k = rot(q)[:, :, q0:q0 + Fq], rot(k)
    # Q: after the rotary, scaled by 32^-0.5 * log2(e) (the kernels' softmax runs in log2 units) -- temporal_layer.hip:1003 (EXT core and
    # fused layer), temporal_layer16.hip:428 / :823 (fused 16 / 13-wave layers), :1150 (13-wave core)
    if defect and "Q" in defect:
        q = _hook(defect, "Q", q * LOG2E, trunc_planes3, 1) / LOG2E
    # K: after the rotary, unscaled -- temporal_layer.hip:776 (EXT), :864 / :926 (fused); temporal_layer16.hip:339 / :860 / :1170
    k = _hook(defect, "K", k, trunc_planes3, 1)
    # V: as projected (loaded) -- temporal_layer.hip:794 (EXT), :889 / :948 (fused); temporal_layer16.hip:355 / :870 / :1157
    v = _hook(defect, "V", v, trunc_planes3, 1)
    i = torch.arange(q0, q0 + Fq)
    j = torch.arange(Fext)
    rel = j[None, :] - i[:, None]
    inside = rel.abs() <= win
    bias = band[(rel.clamp(-win, win) + win)].permute(2, 0, 1)           # (8, Fq, Fext)
    sim = torch.einsum("nhid,nhjd->nhij", q, k) + bias[None]
    sim = sim.masked_fill(~inside[None, None], float("-inf"))
    if defect and "P" in defect:
        # P: split BEFORE the normalisation, which divides P.V by the sum of the unsplit P -- temporal_layer.hip:1079, temporal_layer16.hip:559
        # / :975 / :1279.  The 32 x 32 kernels (temporal_layer.hip) take 2^(s - m) against a running max (half A, then both halves, with
        # alpha rescaling the half-A sum, :1155-1163); here exp(s - row max), which has the defect's size and sign, not the kernel's bits
        e = torch.exp(sim - sim.amax(-1, keepdim=True))
        o = torch.einsum("nhij,nhjd->nhid", _hook(defect, "P", e, trunc_planes3, 1), v) / e.sum(-1, keepdim=True)
    else:
        o = torch.einsum("nhij,nhjd->nhid", sim.softmax(dim=-1), v)      # (HW, 8, Fq, 32)
    return o.permute(2, 0, 1, 3).reshape(Fq * HW, 256).contiguous()


def temporal_layer64(x, Fext, HW, q0, Fq, win, wqkv, wout, rcos, rsin, band, eps=1e-5, defect=None):
    """RefOps.temporal_layer_c64 in float64 with hooks on X, Q, K, V, P and O (packed weights as RefOps takes them)."""
    from oracle.ops_ref import RefOps
    ops = RefOps()
    x = x.double()
    stats = ops.ln_rowstats(x, None, eps)
    if defect and "X" in defect:
        # X: the LayerNorm'ed rows, split by ROUNDING (dawn_split3_rne_quad's bf16 conversions: planes3, not dawn_split3_oct) --
        # the LayerNorm prologues of temporal_layer.hip and temporal_layer16.hip; stale = the third plane of the previous frame row
        xn = ((x - stats[0][:, None]) * stats[1][:, None]).view(Fext, HW, 64)
        xn = _hook(defect, "X", xn, planes3, 0).view(Fext * HW, 64)
        qkv = ops.conv_gemm(xn, wqkv.double(), 768, F=Fext, Hi=1, Wi=HW)
    else:
        qkv = ops.conv_gemm(x, wqkv.double(), 768, row_stats=stats, F=Fext, Hi=1, Wi=HW)
    o = attn_core64(qkv, Fext, HW, q0, Fq, win, rcos, rsin, band, defect)
    # O: after the 1 / l normalisation, before the out-projection -- temporal_layer.hip:1185, temporal_layer16.hip:613 / :1001
    o = _hook(defect, "O", o.view(Fq * HW, 8, 32), trunc_planes3, 1).reshape(Fq * HW, 256)
    return ops.conv_gemm(o, wout.double(), 64, res=x[q0 * HW:(q0 + Fq) * HW], F=Fq, Hi=1, Wi=HW)


def temporal_layer64_segmented(x, Fext, HW, q0, Fq, win, wqkv, wout, rcos, rsin, band, eps=1e-5, defect=None):
    """RefOps.temporal_layer_c64_segmented (its 120-query segments) over temporal_layer64."""
    from oracle.ops_ref import RefOps
    out = torch.empty(Fq * HW, 64, dtype=torch.float64)
    for a in range(q0, q0 + Fq, RefOps.SEG_QUERIES):
        b = min(a + RefOps.SEG_QUERIES, q0 + Fq)
        r0, r1 = max(0, a - win), min(Fext, b + win)
        out[(a - q0) * HW:(b - q0) * HW] = temporal_layer64(x[r0 * HW:r1 * HW], r1 - r0, HW, a - r0, b - a, win, wqkv, wout, rcos, rsin,
                                                            band, eps, defect)
    return out


# ---------------------------------------------------------------------------------------------- inputs
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def coherent(w):
    """w with its three bf16 planes pinned: w1 = the bf16 value in the lowest 16th of w's binade, w2 and w3 each just under half an
    ulp of the plane above, all with w's sign.  Exact in fp32 (24 significant bits), and pack_bf3 splits it back into those planes."""
    w = w.float()
    e = torch.floor(torch.log2(w.abs().clamp_min(1e-30)))
    k = torch.floor((w.abs() / torch.exp2(e) - 1.0) * 16.0)                # 0..15
    m = torch.exp2(e) * (1.0 + k / 128.0) + torch.exp2(e - 9) * 1.96875 + torch.exp2(e - 18) * 1.96875
    return torch.where(w == 0, w, torch.sign(w) * m)


def packd(w_kn):
    """(K, N) -> [K/4][N][4] in the dtype of w_kn (pack_kn, without its cast to fp32)."""
    K, N = w_kn.shape
    return w_kn.reshape(K // 4, 4, N).permute(0, 2, 1).contiguous()


def spread(x):
    """The existing 3x3 gates' data: a few entries x1e4 and x1e-6 -- the split must stay exact across 10 decades."""
    x = x.clone()
    x[::7, ::5] *= 1.0e4
    x[::11, ::3] *= 1.0e-6
    return x


def by_pixels(fn, qkv, F, HW, Fo, chunk=16):
    """fn(qkv of `chunk` pixel columns, chunk) -> (Fo * chunk, 256), over all HW columns of a (F * HW, 768) qkv tensor: the temporal
    attention of a column sees only that column, and a float64 score tensor of every column at once would take gigabytes."""
    out = torch.empty(Fo, HW, 256, dtype=qkv.dtype)
    x = qkv.view(F, HW, 768)
    for a in range(0, HW, chunk):
        b = min(a + chunk, HW)
        out[:, a:b] = fn(x[:, a:b].reshape(F * (b - a), 768), b - a).view(Fo, b - a, 256)
    return out.view(Fo * HW, 256)


def rope(F):
    ang = torch.arange(F).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


class Case:
    def __init__(self, name, kind, split=("w",), form=None, c=C_GATE, **p):
        self.name, self.kind, self.split, self.form, self.c, self.p = name, kind, tuple(split), form, c, p

    def __repr__(self):
        return self.name

    def with_frames(self, F):
        """The same case on fewer frames (the CPU discrimination test: H, W and channels stay)."""
        p = dict(self.p)
        if self.kind == "gemm":
            p["M"] = min(p["M"], F * 256)
        elif self.kind == "tattn":
            p["HW"] = min(p["HW"], F)            # (tattn keeps its frames: F is the number of pixel columns here)
        elif "F" in p:
            p["F"] = min(p["F"], F)
        return Case(self.name, self.kind, self.split, self.form, self.c, **p)

    # inputs: T = fp32 tensors / ints the op takes, Wkn = the fp32 weights in (K, N) form (the images the kernel splits)
    def make(self):
        p, k = self.p, self.kind
        if k == "gemm":
            M, C0, C1, N = p["M"], p["C0"], p.get("C1", 0), p["N"]
            x0 = rnd(M, C0, seed=1) * (1.7 if p.get("ln") else 1.0) + (0.4 if p.get("ln") else 0.0)
            T = dict(x0=x0, x1=rnd(M, C1, seed=5) if C1 else None, res=rnd(M, N, seed=3) if p.get("res") else None,
                     bias=rnd(N, seed=4) if p.get("bias") else None)
            return T, dict(w=coherent(rnd(C0 + C1, N, seed=2, scale=(C0 + C1) ** -0.5)))
        if k in ("down", "up"):
            from dawn_pytorch_amd.pack import conv_w_kn, deconv_w_kn_phases
            F, H, C, N = p["F"], p["H"], p["C"], p["N"]
            T = dict(x=rnd(F * H * H, C, seed=2), bias=rnd(N, seed=3))
            if k == "down":
                return T, dict(w=coherent(conv_w_kn(rnd(N, C, 1, 4, 4, seed=1, scale=(C * 16) ** -0.5))))
            return T, dict(w=coherent(deconv_w_kn_phases(rnd(C, N, 1, 4, 4, seed=4, scale=(C * 4) ** -0.5))))
        if k == "conv3":
            F, H, C0, C1, N = p["F"], p["H"], p["C0"], p.get("C1", 0), p["N"]
            x0, x1 = rnd(F * H * H, C0, seed=1), (rnd(F * H * H, C1, seed=6) if C1 else None)
            if p.get("spread"):
                x0, x1 = spread(x0), (spread(x1) if C1 else None)
            return dict(x0=x0, x1=x1), dict(w=coherent(rnd(9 * (C0 + C1), N, seed=2, scale=(9 * (C0 + C1)) ** -0.5)))
        if k in ("temporal", "temporal_seg"):
            Fext, HW, win = p["F"], p["HW"], 40
            rc, rs = rope(Fext)
            T = dict(x=rnd(Fext * HW, 64, seed=1) * 1.3 + 0.2, rc=rc, rs=rs, band=rnd(2 * win + 1, 8, seed=4))
            return T, dict(wqkv=coherent(rnd(64, 768, seed=2, scale=64 ** -0.5)), wout=coherent(rnd(256, 64, seed=3, scale=256 ** -0.5)))
        if k == "sla":
            F, HW = p["F"], p["HW"]
            return (dict(x=rnd(F * HW, 64, seed=1) * 1.3 + 0.2, bias=rnd(64, seed=4)),
                    # (the attention branch x8 against the residual: at x1 a lost plane is diluted below the gate's floor)
                    dict(wqkv=coherent(rnd(64, 768, seed=2, scale=2.0 * 64 ** -0.5)), wout=rnd(256, 64, seed=3, scale=8.0 * 256 ** -0.5)))
        if k == "xattn":
            from oracle.ops_ref import RefOps
            F, HW, C0, C1 = p["F"], p["HW"], p["C0"], p.get("C1", 0)
            kvtab, nulltab = torch.zeros(F, 3, 128), torch.zeros(3, 16)
            for b in range(3):
                RefOps().xattn_prep(rnd(F, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
            T = dict(x=rnd(F * HW, C0, seed=1) * 1.5 + 0.3, x2=rnd(F * HW, C1, seed=2) if C1 else None, g3=rnd(3, 64, seed=4) * 0.2 + 1,
                     qs=rnd(3, 8, seed=5) * 0.2 + 1, kvtab=kvtab, nulltab=nulltab)
            # (not `coherent`: q is L2-normalised per head, so a defect that shrinks every weight alike cancels there)
            Wkn = dict(wq=rnd(C0 + C1, 192, seed=3, scale=(C0 + C1) ** -0.5))
            Wkn.update({f"wo{b}": rnd(64, 64, seed=10 + b, scale=0.125) for b in range(3)})
            return T, Wkn
        if k == "tattn":
            Fext, win = p["F"], 40
            rc, rs = rope(Fext)
            # (N(0, 1) qkv, as test_hip_ops.test_temporal_attn: x2 makes the softmax peakier and CPU fp32's own error twice as large, and
            # halves the gate's margin over a lost P plane)
            return dict(qkv=rnd(Fext * p["HW"], 768, seed=1), rc=rc, rs=rs, band=rnd(2 * win + 1, 8, seed=4)), {}
        if k in ("sla_unfused", "frame"):
            return dict(qkv=rnd(p["F"] * p["HW"], 768, seed=1)), {}
        if k == "xattn_unfused":
            from oracle.ops_ref import RefOps
            F, HW, Co = p["F"], p["HW"], p["Co"]
            kvtab, nulltab = torch.zeros(F, 3, 128), torch.zeros(3, 16)
            for b in range(3):
                RefOps().xattn_prep(rnd(F, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
            T = dict(q=rnd(F * HW, 192, seed=1), g3=rnd(3, Co, seed=4) * 0.2 + 1, qs=rnd(3, 8, seed=5) * 0.2 + 1, kvtab=kvtab, nulltab=nulltab,
                     y3=rnd(F * HW, 3 * Co, seed=6) * 0.5 + 0.1)
            return T, {f"wo{b}": rnd(64, Co, seed=10 + b, scale=0.125) for b in range(3)}
        raise ValueError(k)

    def ref(self, ops, T, Wkn, dtype):
        """The RefOps op of this case, every floating tensor cast to dtype (float64: want64; float32: base32)."""
        T = {k_: (v.to(dtype) if torch.is_tensor(v) else v) for k_, v in T.items()}
        W = {k_: v.to(dtype) for k_, v in Wkn.items()}
        p, k = self.p, self.kind
        if k == "gemm":
            M, H = p["M"], p.get("H", 16)          # (rows as frames of H x H pixels: a 1x1 projection sees rows only)
            return ops.conv_gemm(T["x0"], packd(W["w"]), p["N"], in1=T["x1"], F=M // (H * H), Hi=H, Wi=H, res=T["res"], bias=T["bias"],
                                 ln_eps=1e-5 if p.get("ln") else 0.0)
        if k == "down":
            H = p["H"]
            return ops.conv_gemm(T["x"], packd(W["w"]), p["N"], F=p["F"], Hi=H, Wi=H, Ho=H // 2, Wo=H // 2, KH=4, KW=4, stride=2, pad=1,
                                 bias=T["bias"])
        if k == "up":
            H = p["H"]
            return ops.conv_gemm(T["x"], torch.stack([packd(W["w"][i]) for i in range(4)], 0), p["N"], F=p["F"], Hi=H, Wi=H, Ho=2 * H,
                                 Wo=2 * H, KH=2, KW=2, mode=1, bias=T["bias"])
        if k == "conv3":
            H = p["H"]
            return ops.conv_gemm(T["x0"], packd(W["w"]), p["N"], in1=T["x1"], F=p["F"], Hi=H, Wi=H, KH=3, KW=3, pad=1)
        if k in ("temporal", "temporal_seg"):
            q0, Fq = p.get("q0", 0), p.get("Fq", p["F"])
            fn = ops.temporal_layer_c64_segmented if k == "temporal_seg" else ops.temporal_layer_c64   # (segments rotate with their own positions)
            return fn(T["x"], p["F"], p["HW"], q0, Fq, 40, packd(W["wqkv"]), packd(W["wout"]), T["rc"], T["rs"],
                                          T["band"])
        if k == "sla":
            return ops.sla_layer_c64(T["x"], p["F"], p["HW"], packd(W["wqkv"]), packd(W["wout"]), T["bias"])
        if k == "tattn":
            Fext, HW, q0 = p["F"], p["HW"], p.get("q0", 0)
            Fq = p.get("Fq", Fext)
            return by_pixels(lambda qkv, n: ops.temporal_attn(qkv, Fext, n, q0, Fq, 40, T["rc"], T["rs"], T["band"]), T["qkv"], Fext, HW, Fq)
        if k == "sla_unfused":
            return ops.sla(T["qkv"], p["F"], p["HW"])
        if k == "frame":
            return ops.frame_attn(T["qkv"], p["F"], p["HW"])
        if k == "xattn_unfused":
            HW, Co, form = p["HW"], p["Co"], p["chain"]
            if form == "ln_sum":
                return ops.xattn_ln_sum(T["y3"], T["g3"], Co)
            o = ops.xattn_core(T["q"].clone(), HW, T["kvtab"], T["nulltab"], T["qs"])
            if form == "core":
                return o
            # "sigma": the original chain (core, the three to_out projections, their LayerNorms, the branch sum) that the per-clip tables
            # of xattn_tables and the one-pass xattn_sigma_out replace
            y3 = torch.cat([o[:, 64 * b:64 * b + 64] @ W[f"wo{b}"] for b in range(3)], 1)
            return ops.xattn_ln_sum(y3, T["g3"], Co)
        if k == "xattn":
            return ops.xattn_layer_c64(T["x"], T["x2"], p["HW"], packd(W["wq"]), [packd(W[f"wo{b}"]) for b in range(3)], T["g3"], T["qs"],
                                       T["kvtab"], T["nulltab"])
        raise ValueError(k)

    def ref_hooked(self, T, Wkn, defect=None):
        """The float64 op of a temporal / temporal_seg / tattn case through the hooked references, `defect` applied."""
        p, k = self.p, self.kind
        q0, Fq = p.get("q0", 0), p.get("Fq", p["F"])
        if k == "tattn":
            return by_pixels(lambda qkv, n: attn_core64(qkv, p["F"], n, q0, Fq, 40, T["rc"], T["rs"], T["band"], defect), T["qkv"].double(),
                             p["F"], p["HW"], Fq)
        fn = temporal_layer64_segmented if k == "temporal_seg" else temporal_layer64
        return fn(T["x"], p["F"], p["HW"], q0, Fq, 40, packd(Wkn["wqkv"]), packd(Wkn["wout"]), T["rc"], T["rs"], T["band"], defect=defect)

    def base32(self, ops, T, Wkn):
        """The op in float32 on CPU, convolutions through torch's im2col + GEMM path (oneDNN and NNPACK off)."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.backends.mkldnn.flags(enabled=False), torch.backends.nnpack.flags(enabled=False):
                return self.ref(ops, T, Wkn, torch.float32)

    def mutant(self, Wkn, defect):
        """Wkn with `defect` (drop_third / stale_third) applied to every weight the kernel splits (float64)."""
        return {k_: (defect(v) if k_ in self.split else v.double()) for k_, v in Wkn.items()}


NONE, TILED, ROWREG, ROWACC, RESAMPLE = 0, 1, 2, 3, 4    # dawn_gemm1x1_form
DIRECT, WINO, WINO4 = 0, 1, 2                         # dawn_conv3x3_form
# dawn_conv3x3_direct_form, which dawn_conv3x3_form = 0 leaves open: a case with `direct` asserts that the answer is one of these
DIRECT_NONE, V2 = 0, (2, 3)                           # the fp32 kernels are next; conv3x3_bf16_v2_kernel, 256 x 64 / 256 x 128 tiles

# Gate factors widened past C_GATE, per kernel: the GPU error / CPU fp32 error measured on an MI355X (max over that kernel's cases).
# Each kernel accumulates K in fp32 on the matrix pipe, one chain of 6 K / 16 MFMA additions per output (CPU GEMM blocks its sums):
C_TILED = 5.0         # gemm1x1_bf16_kernel: 3.7 (K = 512 / 256 with independent random weights; 2.0 with `coherent` ones); the M = 6400 / 25600
                      # cases 2.03 (tiled_M6400_N768_K512_res; 1.61 M6400_N512_K256, 1.32 M25600_N768_K256_res, 0.64 the 256 x 64 plan at K = 96)
C_ROWREG = 3.0        # gemm1x1_rowreg_kernel: 2.0; the K = 64 cases 0.97 (rowreg_M25600_N192_K64+64_ln; 0.94 M25600_N128_K64, 0.91 M6400_N192_K64_ln)
C_ROWACC = 4.0        # gemm1x1_rowacc_kernel: 2.8; 1.75 (rowacc_M25600_N128_K512), 1.48 (rowacc_M6400_N64_K256)
C_ROWACC_LN = 8.0     # ... with the LayerNorm inside: 6.2 when the factor was set -- its statistics sweep takes shifted one-pass sums in fp32 (s2 / K -
                      # md^2 of d = x - shift) over K channels of mean 0.4, std 1.7, where the CPU reference subtracts the mean first.  With the row's
                      # first channel as the shift, rowacc_M6400_N192_K512+512_ln (K = 1024) measured 9.31 and rowacc_M12800_N192_K512_ln 4.00: a row
                      # whose first channel lies 3..4 sigma off its mean cancels, 1 / sigma off by 5.0e-6 / 3.2e-6 of its value (the sweep emulated in
                      # fp32 on the CPU gives 3.1e-6 / 1.6e-6 of the 3.7e-6 / 1.6e-6 measured) -- past 0.8 x the weakest plane defect (11.6 x fp32), so
                      # no tolerance: the kernel's shift is now the mean of the first 16 channels.  Since then 3.66 (K = 1024), 1.87 (K = 512)
C_RESAMPLE = 9.0      # gemm1x1_rowacc_kernel, Downsample / Upsample modes: 7.0 (Downsample, K = 4096), 4.6 (Upsample, K = 1024); at 64 channels of
                      # configs[1]'s first pair 3.79 (down_32x32_C64, K = 1024), 2.87 (up_16x16_C64, K = 256)
C_WINO4 = 8.5         # conv3x3_wino4_kernel: 7.8 (32 x 32, 128 channels; the F(4x4) transform adds values of different magnitude in fp32; the shipped gate
                      # against the GPU's own fp32-MFMA kernel allows 5x).  The narrowest case of the file: its own error is a third of the
                      # largest defect a weight pattern can make (2^-17), so c must sit between 7.8 and ~9 (test_split_gate_cpu).  The 32-wide
                      # template at 64 channels: 5.28 (wino4_32x32_C64+64_N64_n01; 3.97 C64_N64_n01, 3.77 / 2.34 their spread forms)
C_WINO4_K288 = 5.0    # ... at two chunks (wino4_64x64_C32_N64, K = 288): 3.03 (n01; 2.54 spread) x 1.5 = 4.55.  Its own factor because its chain is the
                      # shortest the kernel runs, and C_WINO4 = 8.5 would stand above 0.8 x the weakest plane defect of its spread form (8.7 x CPU
                      # fp32: the cap is 7.0), where the gate could pass a kernel that lost a plane
C_WINO = 5.5          # conv3x3_wino_kernel: 4.2 (the shipped gate against the GPU's direct split kernel allows 3x); the 32 / 16 / 8-wide cases at
                      # 64 .. 512 channels 2.75 (wino_8x8_C256+256_N128_spread; 2.15 its n01 form, 0.61 .. 1.81 the others)
C_SLA_CTX = 3.0       # sla_context_kernel + sla_apply_kernel (fp32, no split operands): 2.46 at HW 1024 (0.94 at 256, 1.07 at 64) -- each context
                      # row is one fp32 MFMA chain over all HW pixels, its softmax denominator one sequential sum of HW / 2 terms per lane
C_DIRECT_DEEP = 11.0  # conv3x3_bf16_v2_kernel on 4 x 4-pixel frames, K = 4608 / 9216: 9.2 -- one chain over all 9 Cin products of an
                      # output, where the Winograd forms at the same channel counts sum over Cin only (3.5 there)
# ... at K = 2304 (256 channels), the same chain at half / a quarter of the length: factors of its own by the rule (measured x 1.5, rounded up to the
# next 0.5), because C_DIRECT_DEEP stands above 0.8 x the weakest plane defect of three of the four cases (test_split_gate_cpu: 12.4 / 14.5 x CPU
# fp32 the n01 forms, 10.5 / 6.1 the spread forms, the least of 8 and 16 CPU threads -- the caps are 9.9 and 4.9).  n01: 5.33 (direct_4x4_C256_N512;
# 4.70 N256).  spread: 2.34 (direct_4x4_C256_N256; 2.08 N512) -- there the largest outputs are those of the few x 1e4 inputs, a handful of products
# each, and the error relative to them is not the long chain's; CPU fp32's own error on that data is 1.5x its n01 one, which halves the cap
C_DIRECT_K2304 = 8.0
C_DIRECT_K2304_SPREAD = 4.0
# The fp32-MFMA kernels that take the convs of an odd clip length hold C_GATE: 1.73 (fp32/conv3x3_8x8_C256_N256_F5), 1.42 (fp32/conv3x3_4x4_C512_N512_F5),
# 2.14 (fp32/gemm1x1_M320_N768_K512_res: 4.65e-7 against 2 x 2.18e-7 + FLOOR = 5.35e-7)

# deepest-level channel counts (512 -> 512 at 8 x 8 and 4 x 4, 512 + 512 -> 256) put K at 4608 / 9216
CASES = [
    # 1x1 family (M = rows; 256 rows = one 16 x 16 frame)
    Case("gemm1x1/tiled_M12800_N768_K512_res", "gemm", form=TILED, c=C_TILED, M=12800, C0=512, N=768, res=True),
    Case("gemm1x1/tiled_M51200_N768_K256", "gemm", form=TILED, c=C_TILED, M=51200, C0=256, N=768),
    Case("gemm1x1/tiled_nS1_M12800_N128_K32", "gemm", form=TILED, c=C_TILED, M=12800, C0=32, N=128, bias=True),
    Case("gemm1x1/tiled_nS2_M12800_N128_K64", "gemm", form=TILED, c=C_TILED, policy=TILED_ONLY, M=12800, C0=64, N=128),
    Case("gemm1x1/tiled_nS3_M12800_N128_K96", "gemm", form=TILED, c=C_TILED, M=12800, C0=96, N=128, res=True),
    # nine stages, the source switch after stage 5 (test_hip_ops.test_gemm1x1_split_variants' M = 25600 form of it runs on the fp32 kernel)
    Case("gemm1x1/tiled_nS9_M12800_N256_K160+128", "gemm", form=TILED, c=C_TILED, M=12800, C0=160, C1=128, N=256, res=True),
    Case("gemm1x1/rowreg_M51200_N64_K128", "gemm", form=ROWREG, c=C_ROWREG, M=51200, C0=128, N=64),
    Case("gemm1x1/rowreg_M51200_N768_K128_ln", "gemm", form=ROWREG, c=C_ROWREG, M=51200, C0=128, N=768, ln=True),
    Case("gemm1x1/rowacc_M51200_N128_K256", "gemm", form=ROWACC, c=C_ROWACC, M=51200, C0=256, N=128),
    Case("gemm1x1/rowacc_M12800_N192_K512_ln", "gemm", form=ROWACC, c=C_ROWACC_LN, M=12800, C0=512, N=192, ln=True),
    # ... at the other launch classes of the two configurations: M = 6400 (configs[1]'s deepest level; fewer workgroups than CUs, or barely more)
    # and M = 25600.  (M / 256) (N / 128) = 150 and 100 wide tiles at M = 6400, which gemm1x1_split_plan turns into 128 x 64 tiles (its plan 3,
    # M <= 12800): 600 and 400 workgroups, two per CU
    Case("gemm1x1/tiled_M6400_N768_K512_res", "gemm", form=TILED, c=C_TILED, M=6400, C0=512, N=768, res=True),
    Case("gemm1x1/tiled_M6400_N512_K256", "gemm", form=TILED, c=C_TILED, M=6400, C0=256, N=512),
    # the 256 x 64 plan (gemm1x1_split_plan answers 1): N % 128 == 0 with t2 = (M / 256) (N / 128) = 100 < 128 wide tiles gives plan 1, and none
    # of plan 3's conditions (N % 128 != 0, M <= 12800, N == 128 with M >= 204800) holds at M = 25600 -- launch_gemm1x1_bf16<1>, 200 workgroups
    # of 256 x 64.  K = 96 keeps the row kernels away (rowreg: K = 64 / 128, rowacc: K >= 256)
    Case("gemm1x1/tiled_plan1_M25600_N128_K96", "gemm", form=TILED, c=C_TILED, M=25600, C0=96, N=128),
    # the 256 x 128 plan with more tiles than CUs (t2 = 600 >= 256)
    Case("gemm1x1/tiled_M25600_N768_K256_res", "gemm", form=TILED, c=C_TILED, M=25600, C0=256, N=768, res=True),
    Case("gemm1x1/rowreg_M6400_N192_K64_ln", "gemm", form=ROWREG, c=C_ROWREG, M=6400, C0=64, N=192, ln=True),
    Case("gemm1x1/rowreg_M25600_N128_K64", "gemm", form=ROWREG, c=C_ROWREG, M=25600, C0=64, N=128),
    Case("gemm1x1/rowreg_M25600_N192_K64+64_ln", "gemm", form=ROWREG, c=C_ROWREG, M=25600, C0=64, C1=64, N=192, ln=True),
    Case("gemm1x1/rowacc_M6400_N192_K512+512_ln", "gemm", form=ROWACC, c=C_ROWACC_LN, M=6400, C0=512, C1=512, N=192, ln=True),
    Case("gemm1x1/rowacc_M6400_N64_K256", "gemm", form=ROWACC, c=C_ROWACC, M=6400, C0=256, N=64),
    Case("gemm1x1/rowacc_M25600_N128_K512", "gemm", form=ROWACC, c=C_ROWACC, M=25600, C0=512, N=128),
    # resample forms of the row-accumulator kernel at configs[2]'s three level pairs (M >= 12800 output / input rows)
    Case("resample/down_64x64_C64", "down", form=RESAMPLE, c=C_RESAMPLE, F=13, H=64, C=64, N=64),
    Case("resample/down_32x32_C128", "down", form=RESAMPLE, c=C_RESAMPLE, F=50, H=32, C=128, N=128),
    Case("resample/down_16x16_C256", "down", form=RESAMPLE, c=C_RESAMPLE, F=200, H=16, C=256, N=256),
    Case("resample/up_8x8_C256", "up", form=RESAMPLE, c=C_RESAMPLE, F=200, H=8, C=256, N=256),
    Case("resample/up_16x16_C128", "up", form=RESAMPLE, c=C_RESAMPLE, F=50, H=16, C=128, N=128),
    Case("resample/up_32x32_C64", "up", form=RESAMPLE, c=C_RESAMPLE, F=13, H=32, C=64, N=64),
    # ... and configs[1]'s first pair (128 px: 64 channels at 32 x 32 / 16 x 16, which configs[2] has at 64 x 64 / 32 x 32)
    Case("resample/down_32x32_C64", "down", form=RESAMPLE, c=C_RESAMPLE, F=50, H=32, C=64, N=64),
    Case("resample/up_16x16_C64", "up", form=RESAMPLE, c=C_RESAMPLE, F=50, H=16, C=64, N=64),
    # 3x3 family at production geometry, N(0,1) data and data spread over 10 decades
    *[Case(f"conv3x3/{nm}_{'spread' if s else 'n01'}", "conv3", form=fm, c=cg[s] if isinstance(cg, tuple) else cg, spread=s, **kw)
      for s in (False, True) for nm, fm, cg, kw in (
        ("wino4_64x64_C64_N64", WINO4, C_WINO4, dict(F=2, H=64, C0=64, N=64)),
        ("wino4_32x32_C128_N128", WINO4, C_WINO4, dict(F=4, H=32, C0=128, N=128)),
        ("wino_64x64_C64+64_N64", WINO, C_WINO, dict(F=2, H=64, C0=64, C1=64, N=64)),
        ("wino_16x16_C512_N128", WINO, C_WINO, dict(F=8, H=16, C0=512, N=128)),
        ("wino_8x8_C512_N512", WINO, C_WINO, dict(F=8, H=8, C0=512, N=512)),
        ("wino_8x8_C512+512_N256", WINO, C_WINO, dict(F=8, H=8, C0=512, C1=512, N=256)),
        ("direct_4x4_C512_N512", DIRECT, C_DIRECT_DEEP, dict(F=32, H=4, C0=512, N=512)),
        ("direct_4x4_C512+512_N256", DIRECT, C_DIRECT_DEEP, dict(F=32, H=4, C0=512, C1=512, N=256)),
        # the other geometries that launch (F = the fewest frames with M % 256 == 0, at least two tiles and F % nf == 0).  F(2x2): TR = 256 / W
        # rows per tile, nf = TR / H frames per tile once a frame is smaller than a tile (8 x 8: nf = 4); the chunk count (C0 + C1) / 16 and the
        # chunk of the source switch (C0 / 16) differ from the cases above
        ("wino_32x32_C128+128_N64", WINO, C_WINO, dict(F=1, H=32, C0=128, C1=128, N=64)),
        ("wino_32x32_C128+128_N128", WINO, C_WINO, dict(F=1, H=32, C0=128, C1=128, N=128)),
        ("wino_16x16_C64_N128", WINO, C_WINO, dict(F=4, H=16, C0=64, N=128)),
        ("wino_16x16_C128+128_N64", WINO, C_WINO, dict(F=4, H=16, C0=128, C1=128, N=64)),
        ("wino_16x16_C256_N256", WINO, C_WINO, dict(F=4, H=16, C0=256, N=256)),
        ("wino_8x8_C256_N256", WINO, C_WINO, dict(F=16, H=8, C0=256, N=256)),
        ("wino_8x8_C256+256_N128", WINO, C_WINO, dict(F=16, H=8, C0=256, C1=256, N=128)),
        ("wino_8x8_C128_N128", WINO, C_WINO, dict(F=8, H=8, C0=128, N=128)),
        # F(4x4), 32-wide template at configs[1]'s level 0 (four and eight chunks, one channel tile); 64-wide with the shortest K it takes
        # (two chunks), which only WINO4_ALL_SHAPES routes there
        ("wino4_32x32_C64_N64", WINO4, C_WINO4, dict(F=1, H=32, C0=64, N=64)),
        ("wino4_32x32_C64+64_N64", WINO4, C_WINO4, dict(F=1, H=32, C0=64, C1=64, N=64)),
        ("wino4_64x64_C32_N64", WINO4, C_WINO4_K288, dict(F=1, H=64, C0=32, N=64, policy=ConvPolicy.WINO4_EVERYWHERE)),
        # the direct v2 kernel's 36-segment form (nf = 16 frames of 4 x 4 pixels per tile) at K = 2304: (n01, spread) factors
        ("direct_4x4_C256_N256", DIRECT, (C_DIRECT_K2304, C_DIRECT_K2304_SPREAD), dict(F=32, H=4, C0=256, N=256, direct=V2)),
        ("direct_4x4_C256_N512", DIRECT, (C_DIRECT_K2304, C_DIRECT_K2304_SPREAD), dict(F=32, H=4, C0=256, N=512, direct=V2)))],
    # odd clip lengths (F % 4 != 0): M % 256 != 0 at the 8 x 8 and 4 x 4 levels, where every conv falls to the fp32-MFMA kernels although
    # all its split images are handed over.  No split operand, no plane defect: held to C_GATE, as the fp32 attention kernels below
    Case("fp32/conv3x3_8x8_C256_N256_F5", "conv3", split=(), form=DIRECT, F=5, H=8, C0=256, N=256, direct=(DIRECT_NONE,)),
    Case("fp32/conv3x3_4x4_C512_N512_F5", "conv3", split=(), form=DIRECT, F=5, H=4, C0=512, N=512, direct=(DIRECT_NONE,)),
    Case("fp32/gemm1x1_M320_N768_K512_res", "gemm", split=(), form=NONE, M=320, H=8, C0=512, N=768, res=True),
    # attention layers
    Case("temporal/F200_q0_w40", "temporal", split=("wqkv", "wout"), F=200, HW=16),
    Case("temporal/shard_F280_q40_Fq200", "temporal", split=("wqkv", "wout"), F=280, HW=16, q0=40, Fq=200),
    Case("temporal/segmented_F400", "temporal_seg", split=("wqkv", "wout"), F=400, HW=8),
    Case("sla/F8_HW256", "sla", split=("wqkv",), F=8, HW=256),
    Case("sla/F9_HW2080", "sla", split=("wqkv",), F=9, HW=2080),
    Case("xattn/C64_HW64", "xattn", split=("wq",), F=3, HW=64, C0=64),
    Case("xattn/C64+64_HW64", "xattn", split=("wq",), F=3, HW=64, C0=64, C1=64),
    Case("xattn/C64_HW4096", "xattn", split=("wq",), F=1, HW=4096, C0=64),
    Case("xattn/C64+64_HW4096", "xattn", split=("wq",), F=1, HW=4096, C0=64, C1=64),
    # the attention core of the unfused levels (HipOps.temporal_attn).  Frames as in production (win 40); the pixel columns shrink only
    # while the automatic kernel stays the same: the split-operand EXT core (dawn_temporal_attn_bf16_try) from 128 columns, below that
    # temporal_attn_kernel (fp32 MFMA)
    Case("tattn/L1_256px_F200", "tattn", split=(), F=200, HW=256),                          # 32 x 32 and 16 x 16 levels at 256 px (FAC = 200)
    Case("tattn/tshard_F280_q40_Fq200", "tattn", split=(), F=280, HW=128, q0=40, Fq=200),   # T-shard interior rank, long-clip row window (FAC = 0)
    Case("tattn/delta7_F200_q47_Fq120", "tattn", split=(), F=200, HW=128, q0=47, Fq=120),   # (q0 - win) mod 16 = 7
    Case("tattn/fp32_256px_F200", "tattn", split=(), F=200, HW=64),                         # 8 x 8 at 256 px: the fp32 kernel
    Case("tattn/fp32_128px_F200", "tattn", split=(), F=200, HW=16),                         # 4 x 4 at 128 px
    # the fp32 attention kernels (no split operands): ops.sla at the levels above 64 channels, ops.frame_attn (the mid level), the unfused
    # cross-attention chain at the channel counts and grids of the two benchmark resolutions
    Case("sla_unfused/HW1024", "sla_unfused", split=(), c=C_SLA_CTX, F=4, HW=1024),
    Case("sla_unfused/HW256", "sla_unfused", split=(), c=C_SLA_CTX, F=8, HW=256),
    Case("sla_unfused/HW64", "sla_unfused", split=(), c=C_SLA_CTX, F=32, HW=64),
    Case("frame/N64", "frame", split=(), F=50, HW=64),
    Case("frame/N16", "frame", split=(), F=100, HW=16),
    *[Case(f"xattn_unfused/{form}_Co{Co}_HW{HW}", "xattn_unfused", split=(), F=F, HW=HW, Co=Co, chain=form)
      for form in ("sigma", "ln_sum") for Co, HW, F in ((128, 1024, 2), (256, 256, 4), (512, 64, 8))],
    Case("xattn_unfused/core_HW1024", "xattn_unfused", split=(), F=2, HW=1024, Co=128, chain="core"),
]

# the operands each kernel family splits in the kernel (the weights' planes are covered by `split` and Case.mutant)
ACT_OPERANDS = {"tattn": ("Q", "K", "V", "P"), "temporal": ("X", "Q", "K", "V", "P", "O"), "temporal_seg": ("X", "Q", "K", "V", "P", "O")}

# (case, operand, defect) -> measured defect / CPU fp32 error ratio, for every activation defect that stays at or below the gate's bound
# (test_split_gate_cpu asserts that exactly these are not rejected).  Empty: the smallest ratios, over the cases and the two defects, are
# X 5.1 (rounded split: its third plane has either sign, half the truncated one's size), P 10.9, Q 11.8, K 11.9, V 14.4, O 16.0 -- each
# above C_GATE = 2 with room for the kernels' measured factors
BELOW_FP32_NOISE = {
}
