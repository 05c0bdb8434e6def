"""oracle/ops_ref.RefOps keeps float64 inputs in float64 for every op the fp64 precision gates use (tests/test_hip_fp64_gates.py), and its
float32 results are bit-for-bit those of the reference as it stood before it learned float64 (commit bf46578, read from git history), which
every fp32-tolerance GPU test compares against.  The same for the whole-UNet oracle (oracle/dawn_oracle.unet_forward), which
tests/test_hip_length_gates.py evaluates in float64: float32 bit for bit as in the parent commit, float64 carried through."""
import math
import subprocess
import types

import pytest
import torch

from conftest import ROOT
from dawn_pytorch_amd.pack import pack_kn
from oracle.ops_ref import RefOps

BEFORE = "bf4657832aef7a48962b103a520ea651b1bf1eb3"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 7 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def W(K, N, seed):
    return pack_kn(rnd(K, N, seed=seed, scale=K ** -0.5))


def rope(F):
    ang = torch.arange(F)[:, None] * (10000.0 ** (-torch.arange(16) / 16.0))[None]
    return ang.cos(), ang.sin()


def cases():
    """name -> (op name, positional args, keyword args): every fp32 tensor argument is cast for the float64 call."""
    F, H, Wd, C = 2, 6, 6, 32
    rows = F * H * Wd
    x, x2 = rnd(rows, C, seed=1), rnd(rows, 16, seed=2)
    ph = torch.stack([W(4 * C, C, seed=10 + i) for i in range(4)], 0)
    c = {
        "conv_gemm/3x3_bias_res_tr": ("conv_gemm", (x, W(9 * C, 48, 3), 48),
                                      dict(F=F, Hi=H, Wi=Wd, KH=3, KW=3, pad=1, bias=rnd(48, seed=4), res=rnd(rows, 48, seed=5),
                                           tr=(rnd(rows, 48, seed=6), rnd(48, seed=7), rnd(48, seed=8)))),
        "conv_gemm/1x1_ln_eps_cat": ("conv_gemm", (x, W(C + 16, 64, 9), 64), dict(in1=x2, F=F, Hi=H, Wi=Wd, ln_eps=1e-5)),
        "conv_gemm/1x1_row_stats": ("conv_gemm", (x, W(C, 64, 11), 64), dict(F=F, Hi=H, Wi=Wd, row_stats=(x.mean(1), x.std(1) + 0.5))),
        "conv_gemm/down4x4s2": ("conv_gemm", (x, W(16 * C, C, 12), C), dict(F=F, Hi=H, Wi=Wd, Ho=3, Wo=3, KH=4, KW=4, stride=2, pad=1)),
        "conv_gemm/transposed": ("conv_gemm", (x, ph, C), dict(F=F, Hi=H, Wi=Wd, Ho=2 * H, Wo=2 * Wd, KH=2, KW=2, mode=1,
                                                               bias=rnd(C, seed=13))),
        "ln_rowstats": ("ln_rowstats", (x, x2), {}),
        "gn_coeffs": ("gn_coeffs", (x, rnd(C, seed=14), rnd(C, seed=15), (rnd(C, seed=16), rnd(C, seed=17)), rows), {}),
    }
    Fext, HW, q0, Fq, win = 12, 4, 2, 8, 3
    cs, sn = rope(Fext)
    band = rnd(2 * win + 1, 8, seed=20)
    xt = rnd(Fext * HW, 64, seed=21)
    c["temporal_attn"] = ("temporal_attn", (rnd(Fext * HW, 768, seed=22), Fext, HW, q0, Fq, win, cs, sn, band), {})
    c["temporal_layer_c64"] = ("temporal_layer_c64", (xt, Fext, HW, q0, Fq, win, W(64, 768, 23), W(256, 64, 24), cs, sn, band), {})
    c["sla"] = ("sla", (rnd(3 * 16, 768, seed=25), 3, 16), {})
    c["sla_layer_c64"] = ("sla_layer_c64", (rnd(3 * 16, 64, seed=26), 3, 16, W(64, 768, 27), W(256, 64, 28), rnd(64, seed=29)), {})
    Fn, HWx, Co = 3, 8, 64
    kvtab, nulltab, qs = rnd(Fn, 3, 128, seed=30), rnd(3, 16, seed=31), rnd(3, 8, seed=32).abs() + 0.5
    wo = [W(64, Co, 33 + b) for b in range(3)]
    g3 = rnd(3, Co, seed=36) * 0.2 + 1
    c["xattn_core"] = ("xattn_core", (rnd(Fn * HWx, 192, seed=37), HWx, kvtab, nulltab, qs), {})
    c["xattn_tables"] = ("xattn_tables", (kvtab, nulltab, qs, wo, Co), {})
    c["xattn_ln_sum"] = ("xattn_ln_sum", (rnd(Fn * HWx, 3 * Co, seed=38), g3, Co), {})
    c["xattn_layer_c64"] = ("xattn_layer_c64", (rnd(Fn * HWx, 64, seed=39), rnd(Fn * HWx, 64, seed=40), HWx, W(128, 192, 41), wo, g3, qs,
                                                kvtab, nulltab), {})
    c["xattn_layer_c64/no_x2"] = ("xattn_layer_c64", (rnd(Fn * HWx, 64, seed=42), None, HWx, W(64, 192, 43), wo, g3, qs, kvtab, nulltab),
                                  {})
    return c


CASES = cases()


def cast(v, dt):
    if torch.is_tensor(v):
        return v.to(dt) if v.is_floating_point() else v
    if isinstance(v, (tuple, list)):
        return type(v)(cast(t, dt) for t in v)
    return v


def call(ops, case, dt):
    op, args, kw = case
    return getattr(ops, op)(*cast(args, dt), **cast(kw, dt))       # (the casts copy: in-place ops never touch the case's tensors)


def outputs(r):
    return list(r) if isinstance(r, (tuple, list)) else [r]


@pytest.fixture(scope="module")
def before():
    try:
        src = subprocess.run(["git", "-C", ROOT, "show", f"{BEFORE}:oracle/ops_ref.py"], check=True, capture_output=True, text=True).stdout
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.skip(f"the reference of commit {BEFORE[:7]} is not in this checkout's git history ({e})")
    mod = types.ModuleType("ops_ref_before")
    exec(compile(src, "ops_ref_before.py", "exec"), mod.__dict__)
    return mod.RefOps()


@pytest.mark.parametrize("name", list(CASES))
def test_float64_in_float64_out(name):
    for t in outputs(call(RefOps(), CASES[name], torch.float64)):
        assert t.dtype == torch.float64, (name, t.dtype)


@pytest.mark.parametrize("name", list(CASES))
def test_float32_unchanged(name, before):
    got, want = outputs(call(RefOps(), CASES[name], torch.float32)), outputs(call(before, CASES[name], torch.float32))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32 and torch.equal(g, w), name


def test_float64_agrees_with_float32():
    """(The float64 path computes the same function: within fp32 rounding of the float32 one.)"""
    for name, case in CASES.items():
        for a, b in zip(outputs(call(RefOps(), case, torch.float64)), outputs(call(RefOps(), case, torch.float32))):
            assert float((a - b.double()).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), name


# ---------------------------------------------------------------------------------------------- the whole UNet (oracle/dawn_oracle.py)
ORACLE_BEFORE = "0bc8995ed9e68a7285f400c17f5e70845871d5f7"      # the oracle before unet_forward carried float64


@pytest.fixture(scope="module")
def oracle_before():
    try:
        src = subprocess.run(["git", "-C", ROOT, "show", f"{ORACLE_BEFORE}:oracle/dawn_oracle.py"], check=True, capture_output=True,
                             text=True).stdout
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.skip(f"the oracle of commit {ORACLE_BEFORE[:7]} is not in this checkout's git history ({e})")
    mod = types.ModuleType("dawn_oracle_before")
    exec(compile(src, "dawn_oracle_before.py", "exec"), mod.__dict__)
    return mod


def _tiny_args(tiny, dt):
    g, sd = tiny
    sd = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
    return sd, torch.from_numpy(g["x"]).to(dt), torch.from_numpy(g["time"]), torch.from_numpy(g["cond"]).to(dt)


def test_unet_forward_float32_unchanged(tiny, oracle_before):
    """oracle.dawn_oracle.unet_forward (and its guided form, and the tables it shares with the kernels) in float32: bit for bit the
    oracle of the parent commit on the tiny golden."""
    from oracle import dawn_oracle as O
    sd, x, time, cond = _tiny_args(tiny, torch.float32)
    got, want = O.unet_forward(sd, x, time, cond, win=3), oracle_before.unet_forward(sd, x, time, cond, win=3)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(O.unet_forward_with_cond_scale(sd, x, time, cond, 2.5, win=3),
                       oracle_before.unet_forward_with_cond_scale(sd, x, time, cond, 2.5, win=3))
    for a, b in zip(O.rotary_tables(12) + (O.sinusoidal_emb(time, 16),), oracle_before.rotary_tables(12) + (oracle_before.sinusoidal_emb(time, 16),)):
        assert a.dtype == torch.float32 and torch.equal(a, b)


def test_unet_forward_carries_float64(tiny):
    """float64 state dict and inputs: float64 out, within fp32 rounding of the float32 evaluation; the shared tables stay the fp32 ones."""
    from oracle import dawn_oracle as O
    sd, x, time, cond = _tiny_args(tiny, torch.float64)
    y64 = O.unet_forward(sd, x, time, cond, win=3)
    assert y64.dtype == torch.float64
    y32 = O.unet_forward(*_tiny_args(tiny, torch.float32), win=3)
    d = float((y64 - y32.double()).abs().max())
    assert 0 < d <= 1e-5 * max(1.0, float(y64.abs().max()))
    e64 = O.sinusoidal_emb(time, 16, torch.float64)
    arg = (time.float()[:, None] * torch.exp(torch.arange(8, dtype=torch.float32) * -(math.log(10000) / 7))).double()
    assert e64.dtype == torch.float64 and torch.equal(e64, torch.cat((arg.sin(), arg.cos()), -1))      # fp32 argument, float64 sine
