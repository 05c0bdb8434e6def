"""-m gpu: the kernels of the HuBERT audio-feature stage and of the PBnet pose / blink stage against a float64 reference at fp32 accuracy
(tests/stage_gate.py), at the stages' own shapes: hubert-large's conv_gemm launches (after asserting that they take the generic fp32-MFMA
kernel under the shipped policy), attn64 on both sides of its tile edges at unit scale and at score std 9, the two-pass LayerNorm on
outlier channels, the Cin = 1 first conv, the utterance normalisation, GELU's tails, attn_bias32 under the eval-mode window mask and
dawn_linear at the decoder's shapes.

The gate (split_gate.fp32_gate): max|hip - fp64| / max|fp64| <= c x the same for the RefOps op in fp32 on CPU + FLOOR, c = C_GATE = 2 unless
stage_gate.C_WIDE widens it with the MI355X measurement beside it.  tests/test_stage_gate_cpu.py shows that every case rejects a tf32-class
operand and the structural defects of its kernel.  Each gate appends its errors and its ratio to CPU fp32 to the op-error log."""
import pytest
import torch

import stage_gate as S
from dawn_pytorch_amd.pack import pack_kn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def cu(t):
    return None if t is None else t.cuda()


def of_kind(*kinds):
    cs = [c for c in S.CASES if c.kind in kinds]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def gate(case, got, T):
    torch.cuda.synchronize()
    return S.fp32_gate(case.name, got, case.want64(T), case.base32(T), c=case.c)


@of_kind("hconv")
def test_hubert_conv_gemm_fp64_gate(hip, case):
    """Every conv_gemm launch of HubertFeatures.encode, with its keyword set, under the shipped policy (conv_policy 0)."""
    T, p = case.make(), case.p
    g = p.get("group")
    buf = cu(T["buf"])
    x = buf if g is None else buf[:, g * 64:(g + 1) * 64]
    kw = dict(case.conv_kw(), bias=cu(T["bias"]))
    if T["res"] is not None:
        kw["res"] = cu(T["res"])
    pos = None
    if g is not None:
        pos = torch.full((case.rows_out(), 1024), S.SENTINEL, device="cuda")
        kw["out"] = pos[:, g * 64:(g + 1) * 64]
    w = pack_kn(T["w"]).cuda()
    assert hip.conv_policy == 0
    assert hip.conv_gemm(x, w, p["N"], **kw, form_only=True) == (0, 0), case.name       # the generic fp32-MFMA implicit GEMM
    got = hip.conv_gemm(x, w, p["N"], **kw)
    assert tuple(got.shape) == (case.rows_out(), p["N"])
    gate(case, got, T)
    if g is not None:
        keep = torch.ones(1024, dtype=torch.bool)
        keep[g * 64:(g + 1) * 64] = False
        assert bool((pos.cpu()[:, keep] == S.SENTINEL).all()), f"{case.name}: written outside the group's columns"
        assert torch.equal(buf.cpu(), T["buf"]), f"{case.name}: input buffer modified"


@of_kind("attn64")
def test_attn64_fp64_gate(hip, case):
    T = case.make()
    gate(case, hip.attn64(cu(T["qkv"]), S.HEADS64), T)


@of_kind("ln")
def test_ln_affine_act_fp64_gate(hip, case):
    T = case.make()
    gate(case, hip.ln_affine_act(cu(T["x"]), cu(T["g"]), cu(T["b"]), 1e-5, case.p["act"]), T)


@of_kind("conv0", "wavenorm", "addact")
def test_hubert_pointwise_fp64_gate(hip, case):
    T = case.make()
    if case.kind == "conv0":
        got = hip.hubert_conv0(cu(T["x"]), cu(T["w"]), cu(T["bias"]), 5)
    elif case.kind == "wavenorm":
        got = hip.wave_normalize(cu(T["x"]))
    elif case.p.get("inplace"):
        got = cu(T["b"]).clone()
        hip.add_act(None, got, 2, out=got)
    else:
        got = hip.add_act(cu(T["a"]), cu(T["b"]), 2)
    gate(case, got, T)


@of_kind("attn32")
def test_attn_bias32_fp64_gate(hip, case):
    T = case.make()
    q, k, v = case.qkv32(cu(T["qkv"]))
    gate(case, hip.attn_bias32(q, k, v, S.HEADS32, cu(T["bias"]), cu(T["rc"]), cu(T["rs"]), 32 ** -0.5), T)


@of_kind("linear")
def test_linear_fp64_gate(hip, case):
    T = case.make()
    gate(case, hip.linear(cu(T["x"]), cu(T["W"]), cu(T["bias"]), act_in=case.p["act_in"]), T)
