"""The fp32-accuracy gate of tests/split_gate.py can fail: for every gate case, built with the same inputs and weights as the GPU test
(fewer frames; H, W and channels unchanged), it REJECTS the op computed with each weight the kernel splits
  * truncated to its top two bf16 planes (the a1 . b3 term lost), and
  * given the third plane of another matrix (a stale prefetch),
and ACCEPTS the op evaluated in fp32 on CPU.  The same for the operands the attention kernels split in the kernel (split_gate.ACT_OPERANDS):
each operand with its third plane dropped, or read from the previous head, is REJECTED, unless split_gate.BELOW_FP32_NOISE lists it.  The conv cases without split operands (an odd clip length: the fp32-MFMA kernels)
REJECT weights truncated to 16 mantissa bits, and every conv case reaches, at its GPU shape, the kernel it names (the routing run dry).  No GPU."""
import functools

import pytest
import torch

from oracle.ops_ref import RefOps
import split_gate as G

CPU_FRAMES = {"gemm": 64, "down": 4, "up": 4, "conv3": 32, "temporal": 280, "temporal_seg": 400, "sla": 2, "xattn": 1,     # (conv3: as on the GPU)
              "tattn": 8}                                                                                           # (tattn: pixel columns)
WEIGHT_CASES = [c for c in G.CASES if c.split]


@pytest.mark.parametrize("case", WEIGHT_CASES, ids=[c.name for c in WEIGHT_CASES])
def test_gate_rejects_plane_defects(case):
    case = case.with_frames(CPU_FRAMES[case.kind])
    ops = RefOps()
    T, Wkn = case.make()
    want64 = case.ref(ops, T, Wkn, G.torch.float64)
    base32 = case.base32(ops, T, Wkn)
    assert not G.gate_rejects(base32, want64, base32, c=case.c)
    errs = {"fp32": G.rel_err(base32, want64)}
    for defect in (G.drop_third, G.stale_third):
        mut = case.ref(ops, T, case.mutant(Wkn, defect), G.torch.float64)
        errs[defect.__name__] = G.rel_err(mut, want64)
    bound = case.c * errs["fp32"] + G.FLOOR
    assert errs["drop_third"] > bound and errs["stale_third"] > bound, (case.name, bound, errs)


def test_the_gate_itself():
    t = G.torch.linspace(1.0, 2.0, 100, dtype=G.torch.float64)
    base = t.float()
    G.fp32_gate("self", t.float(), t, base, log=False)
    with pytest.raises(AssertionError):
        G.fp32_gate("self", (t * (1 + 3e-6)).float(), t, base, log=False)
    w = G.coherent(G.rnd(64, 96, seed=3) * 0.1)
    w1, w2, w3 = G.planes3(w)
    assert torch.equal(w1.double() + w2.double() + w3.double(), w.double())              # exact in fp32, split back into its planes
    assert bool((w3 * w > 0).all()) and float((w3 / w).min()) > 6e-6                       # third plane maximal, with the weight's sign
    from dawn_pytorch_amd.pack import pack_bf3
    third = pack_bf3(w)[:, 2].view(torch.bfloat16).float()                                # [K/16][2][N][8] -> (K, N)
    assert torch.equal(third.permute(0, 1, 3, 2).reshape(64, 96), w3)                       # ... the plane the kernels read
    # the in-kernel split of the activation operands: dawn_split3_oct's truncation, emulated exactly
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.randn(4096, generator=g), G.spread(torch.randn(64, 64, generator=g)).flatten(),
                   (torch.rand(1024, generator=g) + 1.0) * 2.0 ** -109 * torch.randn(1024, generator=g).sign()])
    # (subnormal-adjacent: |x| in [2^-109, 2^-108): the last bit of the third plane at 2^-132, just above bf16's subnormal resolution)
    p1, p2, p3 = G.trunc_planes3(x)
    assert torch.equal(p1.double() + p2.double() + p3.double(), x.double())
    for pl in (p1, p2, p3):
        assert torch.equal(pl.to(torch.bfloat16).float(), pl)                          # every piece a bf16 value
    assert bool((p1.abs() >= x.abs() * (1 - 2.0 ** -7)).all()) and bool((p3 * x >= 0).all())     # truncation: all pieces carry x's sign
    # below that, where x - p1 - p2 is subnormal, dawn_split3_oct's top-16-bit truncation of it keeps bf16's subnormal resolution only
    # (2^-133): what the kernels do too (fp32 denormals are not flushed), with no bearing on any activation the network makes
    x = torch.randn(4096, generator=g) * 2.0 ** -120
    p1, p2, p3 = G.trunc_planes3(x)
    lost = x.double() - (p1.double() + p2.double() + p3.double())
    assert bool((lost.abs() < 2.0 ** -133).all()) and bool((lost != 0).any())


# ---------------------------------------------------------------------------------------------- activation planes of the attention kernels
ACT_CASES = [c for c in G.CASES if c.kind in G.ACT_OPERANDS]


@functools.lru_cache(maxsize=None)
def _act_refs(name):
    case = next(c for c in ACT_CASES if c.name == name)
    case = case.with_frames(CPU_FRAMES[case.kind])
    T, Wkn = case.make()
    return case, T, Wkn, case.ref_hooked(T, Wkn), case.base32(RefOps(), T, Wkn)


@pytest.mark.parametrize("case", ACT_CASES, ids=[c.name for c in ACT_CASES])
def test_hooked_reference_is_the_oracle(case):
    """Without hooks, the hooked float64 copy of the attention core / temporal layer is the RefOps op in float64."""
    case, T, Wkn, want64, _ = _act_refs(case.name)
    oracle = case.ref(RefOps(), T, Wkn, torch.float64)
    assert want64.dtype == oracle.dtype == torch.float64
    assert float((want64 - oracle).abs().max() / oracle.abs().max()) <= 1e-14


ACT_PARAMS = [(c, op) for c in ACT_CASES for op in G.ACT_OPERANDS[c.kind]]


@pytest.mark.parametrize("case,operand", ACT_PARAMS, ids=[f"{c.name}-{op}" for c, op in ACT_PARAMS])
def test_gate_rejects_activation_plane_defects(case, operand):
    case, T, Wkn, want64, base32 = _act_refs(case.name)
    assert not G.gate_rejects(base32, want64, base32, c=case.c)
    e32 = G.rel_err(base32, want64)
    bound = case.c * e32 + G.FLOOR
    kept = {}
    for defect in G.ACT_DEFECTS:
        e = G.rel_err(case.ref_hooked(T, Wkn, {operand: defect}), want64)
        if e <= bound:
            kept[defect.__name__] = e / e32
    listed = {d for (c, op, d) in G.BELOW_FP32_NOISE if (c, op) == (case.name, operand)}
    assert set(kept) == listed, (case.name, operand, f"bound {bound:.3e}", kept)


# (and the convs of an odd clip length, which the router hands to the fp32-MFMA kernels: conv3 / gemm cases without split operands)
FP32_CONV_CASES = [c for c in G.CASES if c.kind in ("gemm", "conv3") and not c.split]
FP32_CASES = [c for c in G.CASES if c.kind in ("tattn", "sla_unfused", "frame", "xattn_unfused")] + FP32_CONV_CASES


@pytest.mark.parametrize("case", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_fp32_kernel_cases_have_an_fp32_baseline(case):
    """The gate of a kernel without split operands: its CPU fp32 baseline is a real fp32 error (not 0, not past fp32 accuracy)."""
    case = case.with_frames(CPU_FRAMES.get(case.kind, 2))
    T, Wkn = case.make()
    ops = RefOps()
    e32 = G.rel_err(case.base32(ops, T, Wkn), case.ref(ops, T, Wkn, torch.float64))
    assert 1e-8 < e32 < 2e-6, e32


@pytest.mark.parametrize("case", FP32_CONV_CASES, ids=[c.name for c in FP32_CONV_CASES])
def test_gate_rejects_reduced_precision_weights(case):
    """The fp32 conv cases have no plane to lose; what their gate must see is a matrix pipe of less than fp32 precision: the weights
    truncated to their top 16 mantissa bits (decode_gate.trunc16) are REJECTED, CPU fp32 is accepted."""
    from decode_gate import trunc16
    ops = RefOps()
    T, Wkn = case.make()
    want64 = case.ref(ops, T, Wkn, torch.float64)
    base32 = case.base32(ops, T, Wkn)
    assert not G.gate_rejects(base32, want64, base32, c=case.c)
    mut = case.ref(ops, T, {k: trunc16(v) for k, v in Wkn.items()}, torch.float64)
    assert G.gate_rejects(mut, want64, base32, c=case.c), (case.name, G.rel_err(mut, want64), G.rel_err(base32, want64))


# ---------------------------------------------------------------------------------------------- the kernel each conv case names
CONV_CASES = [c for c in G.CASES if c.kind in ("gemm", "down", "up", "conv3")]


def conv_desc(case):
    """The descriptor HipOps.conv_gemm builds for the case in tests/test_hip_fp64_gates.py (conv_call), on pointers that are never read."""
    from dawn_pytorch_amd import _lib
    FAKE = 0x1000
    p, k = case.p, case.kind
    d = _lib.ConvDesc()
    C0, C1, N = p.get("C0", p.get("C")), p.get("C1", 0), p["N"]
    d.in0, d.C0, d.ld0 = FAKE, C0, C0
    if C1:
        d.in1, d.C1, d.ld1 = FAKE, C1, C1
    d.w, d.w_bf3, d.N, d.out, d.ld_out, d.stride = FAKE, FAKE, N, FAKE, N, 1
    H = p.get("H", 16)
    d.F = p["M"] // (H * H) if k == "gemm" else p["F"]
    d.Hi = d.Wi = d.Ho = d.Wo = H
    if k == "gemm":
        d.KH = d.KW = 1
        if p.get("res"):
            d.res, d.ld_res = FAKE, N
        if p.get("bias"):
            d.bias = FAKE
        if p.get("ln"):
            d.ln_eps = 1e-5
    elif k == "down":
        d.Ho = d.Wo = H // 2
        d.KH, d.KW, d.stride, d.pad, d.bias = 4, 4, 2, 1, FAKE
    elif k == "up":
        d.Ho = d.Wo = 2 * H
        d.KH, d.KW, d.mode, d.bias = 2, 2, 1, FAKE
    else:
        d.KH, d.KW, d.pad, d.w_wino, d.w_wino4 = 3, 3, 1, FAKE, FAKE
    d.policy = int(p.get("policy", 0))
    return d


@pytest.mark.parametrize("case", CONV_CASES, ids=[c.name for c in CONV_CASES])
def test_conv_case_reaches_the_kernel_it_names(case):
    """dawn_conv3x3_form / dawn_gemm1x1_form / dawn_conv3x3_direct_form (host code: the launch's own routing run dry) of every conv case at
    its GPU shape -- what tests/test_hip_fp64_gates.py asserts again on the very descriptor it launches."""
    import ctypes as C
    from dawn_pytorch_amd import _lib
    L, d = _lib.lib(), conv_desc(case)
    forms = (L.dawn_conv3x3_form(C.byref(d)), L.dawn_gemm1x1_form(C.byref(d)))
    assert forms == ((case.form, 0) if case.kind == "conv3" else (0, case.form)), (case.name, forms)
    if "direct" in case.p:
        assert L.dawn_conv3x3_direct_form(C.byref(d)) in case.p["direct"], case.name
