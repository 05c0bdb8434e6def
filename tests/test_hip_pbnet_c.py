"""-m gpu: the windowed PBnet attention (dawn_attn_win32) against the torch op on the dense (heads, Tq, Tk) expansion of its table, against
the dense kernel, against float64 and against itself; and the C-side pose / blink stage (dawn_pbnet_generate / dawn_pose_blink_stage through
ctx.PbnetEvaluator and `via_c=True`) against the reference's own vectors, the pinned CPU oracle, float64 and the Python orchestration.

Measured on an MI355X (tools/bench_pbnet.py has the timings): on every case below dawn_attn_win32 and dawn_attn_bias32 on the expanded table
gave the same bits (`torch.equal`); the test prints the finding per case and requires 2e-5 only."""
import ctypes as C

import pytest
import torch

from conftest import load_golden
from dawn_pytorch_amd import _lib, ctx
from dawn_pytorch_amd.ops import HipOps
from dawn_pytorch_amd.pbnet import PoseBlinkGenerator, pose_blink_stage
from guarded import GuardedOps
from oracle import pbnet_ref as R
from oracle.ops_ref import RefOps
from split_gate import fp32_gate
from stage_gate import attn32_64
from test_hip_ops import check
from test_hip_pbnet import _random_decoder_sd

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
MODELS = {"pose": "transformerreemb6", "blink": "transformerreemb5"}
HEADS, HD, SCALE = 4, 128, 32 ** -0.5

# (Tq, Tk, win): the window never cuts; one and two windows of 100 inside the clip; the same for 200; tiles whose key range is clipped on
# both sides; Tq != Tk; the 64-query / 64-key tile edges; a single query
SHAPES = [(20, 20, 100), (130, 130, 100), (210, 210, 100), (210, 210, 200), (470, 470, 200), (70, 201, 100), (65, 65, 1), (129, 129, 64),
          (1, 5, 3)]


@pytest.fixture(scope="module")
def hip():
    return HipOps()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def expand(bias_rel, Tq, Tk, win, dtype=torch.float32):
    """(heads, 2 win + 1) or None -> the dense (heads, Tq, Tk) table dawn_attn_bias32 takes: -1e8 outside the band."""
    rel = torch.arange(Tk)[None, :] - torch.arange(Tq)[:, None]
    band = rel.abs() <= win
    ex = torch.full((HEADS, Tq, Tk), -1e8, dtype=dtype)
    ex[:, band] = 0 if bias_rel is None else bias_rel.to(dtype)[:, (rel + win)[band]]
    return ex


def rotary(n, nrot):
    if nrot == 0:
        return None, None
    ang = torch.arange(n).float()[:, None] * (1.0 / 10000 ** (torch.arange(nrot).float() / nrot))[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


_cases = {}


def case(Tq, Tk, win, nrot, with_bias, sigma=1.0):
    """Seeded inputs (q | k | v as column slices of one tensor, as the decoder slices its to_qkv output) and the fp32 CPU reference on the
    dense expansion; computed once per module, never modified."""
    key = (Tq, Tk, win, nrot, with_bias, sigma)
    if key not in _cases:
        n = max(Tq, Tk)
        qkv = rnd(n, 3 * HD, seed=Tq + Tk, scale=sigma)
        br = rnd(HEADS, 2 * win + 1, seed=4, scale=1.5) if with_bias else None
        rc, rs = rotary(n, nrot)
        q, k, v = qkv[:Tq, :HD], qkv[:Tk, HD:2 * HD], qkv[:Tk, 2 * HD:]
        dense = expand(br, Tq, Tk, win)
        _cases[key] = dict(qkv=qkv, br=br, rc=rc, rs=rs, dense=dense, want=RefOps().attn_bias32(q, k, v, HEADS, dense, rc, rs, SCALE))
    return _cases[key]


def dev(t):
    return None if t is None else t.cuda()


def run_win(hip, c, Tq, Tk, win, strided, out=None):
    g = c["qkv"].cuda()
    q, k, v = g[:Tq, :HD], g[:Tk, HD:2 * HD], g[:Tk, 2 * HD:]
    if not strided:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return hip.attn_win32(q, k, v, HEADS, win, dev(c["br"]), dev(c["rc"]), dev(c["rs"]), SCALE, out=out)


@pytest.mark.parametrize("Tq,Tk,win", SHAPES)
def test_attn_win32_vs_dense_reference_and_dense_kernel(hip, Tq, Tk, win):
    for nrot in (0, 2, 16):
        for with_bias in (True, False):
            c = case(Tq, Tk, win, nrot, with_bias)
            name = f"attn_win32/{Tq}x{Tk}_w{win}_r{nrot}_b{int(with_bias)}"
            got = run_win(hip, c, Tq, Tk, win, strided=False)
            check(name, got, c["want"], 2e-5)
            g = c["qkv"].cuda()
            dense = hip.attn_bias32(g[:Tq, :HD].contiguous(), g[:Tk, HD:2 * HD].contiguous(), g[:Tk, 2 * HD:].contiguous(), HEADS,
                                    c["dense"].cuda(), dev(c["rc"]), dev(c["rs"]), SCALE)
            check(name + "/vs_dense_kernel", got, dense, 2e-5)
            print(f"{name}: bit-equal to dawn_attn_bias32 on the expanded table: {torch.equal(got, dense)}")
    c = case(Tq, Tk, win, 2, True)
    got = run_win(hip, c, Tq, Tk, win, strided=True)                       # q | k | v as column slices of one tensor
    check(f"attn_win32/{Tq}x{Tk}_w{win}_strided", got, c["want"], 2e-5)
    assert torch.equal(got, run_win(hip, c, Tq, Tk, win, strided=False))


def test_attn_win32_window_zero_is_v(hip):
    Tn = 130
    c = case(Tn, Tn, 0, 2, True)
    got = run_win(hip, c, Tn, Tn, 0, strided=True)
    assert torch.equal(got.cpu(), c["qkv"][:Tn, 2 * HD:])                  # one key: p = 1


@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_attn_win32_fp64_gate(hip, sigma):
    """As stage_gate's attn_bias32 cases (2 rotary pairs, bias of scale 1.5, unit scale and score sigma = 3), with the factor and the floor
    of test_hip_pbnet.py."""
    Tq, Tk, win = 470, 470, 200
    c = case(Tq, Tk, win, 2, True, sigma)
    q, k, v = c["qkv"][:Tq, :HD], c["qkv"][:Tk, HD:2 * HD], c["qkv"][:Tk, 2 * HD:]
    want64 = attn32_64(q, k, v, HEADS, expand(c["br"], Tq, Tk, win, torch.float64), c["rc"], c["rs"], SCALE)
    assert want64.dtype == torch.float64
    fp32_gate(f"attn_win32/{Tq}x{Tk}_w{win}_sigma{sigma:g}", run_win(hip, c, Tq, Tk, win, strided=True), want64, c["want"], c=3.0, floor=2e-6)


def test_attn_win32_refusals_leave_the_output_alone():
    L = _lib.lib()
    x = rnd(40, HD, seed=1).cuda()
    out = torch.full((40, HD), float("nan"), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = x.data_ptr()

    def call(Tq, Tk, win, ldq=HD, ld_out=HD):
        return L.dawn_attn_win32(p, ldq, p, HD, p, HD, Tq, Tk, HEADS, win, None, None, None, 0, SCALE, out.data_ptr(), ld_out, st)
    for args, word in (((40, 30, 9), "without a key"), ((40, 40, -1), "win < 0"), ((40, 40, 5, HD - 1), "strides"),
                       ((40, 40, 5, HD, HD - 1), "strides")):
        assert call(*args) != 0 and word in L.dawn_last_error().decode(), args
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(40, 30, 10) == 0                                           # Tq == Tk + win: the last query still has its key
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())


def test_attn_win32_deterministic(hip):
    c = case(470, 470, 200, 2, True)
    assert torch.equal(run_win(hip, c, 470, 470, 200, strided=True), run_win(hip, c, 470, 470, 200, strided=True))


@pytest.mark.parametrize("Tq,Tk,win", [(130, 130, 100), (70, 201, 100), (65, 65, 1)])
def test_attn_win32_guarded_output(Tq, Tk, win):
    """Poisoned output between bands and column neighbours of a bit pattern (tests/guarded.py): every element written, nothing else."""
    g = GuardedOps()
    c = case(Tq, Tk, win, 2, True)
    out = g.guarded_out(Tq, HD, col_pad=8, name="attn_win32.out")
    assert out.stride(0) == HD + 16
    got = run_win(g, c, Tq, Tk, win, strided=True, out=out)
    g.verify()
    check(f"attn_win32/{Tq}x{Tk}_w{win}_guarded", got, c["want"], 2e-5)
    res = run_win(g, c, Tq, Tk, win, strided=True)                         # the op's own allocation, poisoned by GuardedOps.empty
    g.verify()
    assert torch.equal(res, got)


# ---------------------------------------------------------------------------------------------- the C-side stage
def tiny_gen(g, name):
    sd = {k.split(":", 2)[2]: T_(g[k]) for k in g if k.startswith(f"sd:{name}:")}
    return PoseBlinkGenerator(sd, archiname=MODELS[name], num_heads=int(g["heads"]), device="cuda")


@pytest.mark.parametrize("name", list(MODELS))
def test_via_c_vs_reference_golden(name):
    g = load_golden("pbnet_tiny.npz")
    gen = tiny_gen(g, name)
    for c in ("T20", "T130", "T210"):
        out = gen.generate(T_(g[f"{name}:{c}:init"]), T_(g[f"{name}:{c}:audio"]), T_(g[f"{name}:{c}:dur"]), fact=1, z=T_(g[f"{name}:{c}:z"]),
                           via_c=True)
        assert out["output"].is_cuda and set(out) == {"x", "z", "y", "mask", "lengths", "output"}
        check(f"pbnet_via_c/{name}_{c}", out["output"], T_(g[f"{name}:{c}:out"]), 2e-5)
    assert gen._tables == {}                                               # no (heads, T, T) table was built


_shipped = {}


def shipped(name, Tn):
    """Shipped-size decoder (audio 1024, latent 256, 4 layers, ff 1024; random init), its inputs and the oracle in fp32 and fp64 on the
    CPU; computed once per module."""
    key = (name, Tn)
    if key not in _shipped:
        in_dim, seed = {"pose": (6, 1), "blink": (2, 2)}[name]
        sd = _random_decoder_sd(in_dim, seed=seed)
        gn = torch.Generator().manual_seed(5)
        audio, z, ip = torch.randn(1, Tn, 1024, generator=gn), torch.randn(Tn, 1, 256, generator=gn), torch.rand(1, 1, in_dim, generator=gn)
        dur = torch.tensor([Tn])
        base32 = R.generate(sd, ip, audio, dur, z, archiname=MODELS[name])
        want64 = R.generate({k: v.double() for k, v in sd.items()}, ip.double(), audio.double(), dur, z.double(), archiname=MODELS[name])
        assert want64.dtype == torch.float64 and base32.dtype == torch.float32
        _shipped[key] = dict(sd=sd, audio=audio, z=z, ip=ip, dur=dur, base32=base32, want64=want64)
    return _shipped[key]


@pytest.mark.parametrize("name", list(MODELS))
def test_via_c_shipped_size_T200(name):
    s = shipped(name, 200)
    gen = PoseBlinkGenerator(s["sd"], archiname=MODELS[name], device="cuda")
    got = gen.generate(s["ip"], s["audio"], s["dur"], z=s["z"], via_c=True)["output"]
    assert gen._tables == {}
    check(f"pbnet_via_c_full/{name}", got, s["base32"], 3e-5)
    fp32_gate(f"pbnet_via_c_full/{name}", got, s["want64"], s["base32"], c=3.0, floor=2e-6)
    py = gen.generate(s["ip"], s["audio"], s["dur"], z=s["z"])["output"]
    check(f"pbnet_via_c_full/{name}_vs_python", got, py, 3e-5)
    print(f"pbnet_via_c_full/{name}: max|via_c - python| = {float((got - py).abs().max()):.3e}, equal bits: {torch.equal(got, py)}")
    assert torch.equal(got, gen.generate(s["ip"], s["audio"], s["dur"], z=s["z"], via_c=True)["output"])


@pytest.mark.parametrize("name", list(MODELS))
def test_via_c_shipped_size_T1000_fp64_gate(name):
    """Five (pose) / two and a half (blink) windows: the gate calibrates itself on CPU fp32's own error at this length."""
    s = shipped(name, 1000)
    gen = PoseBlinkGenerator(s["sd"], archiname=MODELS[name], device="cuda")
    got = gen.generate(s["ip"], s["audio"], s["dur"], z=s["z"], via_c=True)["output"]
    assert gen._tables == {}
    fp32_gate(f"pbnet_via_c_T1000/{name}", got, s["want64"], s["base32"], c=3.0, floor=2e-6)


def test_pose_blink_stage_via_c():
    """dawn_pose_blink_stage == the stage on the torch op set (the tolerances of test_hip_pbnet.py), through `via_c=True` and written at
    caller strides into NaN-filled buffers."""
    Tn = 200
    sp, sb = shipped("pose", Tn), shipped("blink", Tn)
    gp = PoseBlinkGenerator(sp["sd"], archiname="transformerreemb6", device="cuda")
    gb = PoseBlinkGenerator(sb["sd"], archiname="transformerreemb5", device="cuda")
    audio, zp, zb = sp["audio"][0], sp["z"], sb["z"]
    init_pose, init_blink = torch.tensor([[3.0, -5.0, 1.0, 4.79e-04, 56.5, 64.9, 9.9]]), torch.tensor([[0.3, 0.28]])
    cp = PoseBlinkGenerator(sp["sd"], archiname="transformerreemb6", ops=RefOps())
    cb = PoseBlinkGenerator(sb["sd"], archiname="transformerreemb5", ops=RefOps())
    wp, wb = pose_blink_stage(cp, cb, audio, init_pose, init_blink, z_pose=zp, z_blink=zb)
    pose, blink = pose_blink_stage(gp, gb, audio, init_pose, init_blink, z_pose=zp, z_blink=zb, via_c=True)
    assert pose.shape == (Tn, 6) and blink.shape == (Tn, 2) and not pose.is_cuda and gp._tables == {} and gb._tables == {}
    torch.testing.assert_close(pose, wp, atol=2e-2, rtol=1e-5)                  # (de-normalised by ranges of up to 1080)
    torch.testing.assert_close(blink, wb, atol=2e-5, rtol=0)
    # a host aims the stage at its own buffer: the pose / blink columns of a (T, 11) block
    block = torch.full((Tn, 11), float("nan"), device="cuda")
    ctx.pose_blink_stage_c(gp.c_evaluator(), gb.c_evaluator(), audio.cuda(), init_pose[0, :6], init_blink[0, :2], zp[:, 0].contiguous().cuda(),
                           zb[:, 0].contiguous().cuda(), dri_pose=block[:, 1:7], dri_blink=block[:, 8:10])
    assert torch.equal(block[:, 1:7].cpu(), pose) and torch.equal(block[:, 8:10].cpu(), blink)
    assert bool(torch.isnan(block[:, [0, 7, 10]]).all())
    # without injected latents the draw is the default path's: pose first, then blink, from torch's global generator
    torch.manual_seed(11)
    a = pose_blink_stage(gp, gb, audio, init_pose, init_blink, via_c=True)
    torch.manual_seed(11)
    z1, z2 = torch.randn(Tn, 1, 256, device="cuda"), torch.randn(Tn, 1, 256, device="cuda")
    b = pose_blink_stage(gp, gb, audio, init_pose, init_blink, z_pose=z1, z_blink=z2, via_c=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_stage_refusals_leave_the_outputs_alone():
    L = _lib.lib()
    g = load_golden("pbnet_tiny.npz")
    evp, evb = tiny_gen(g, "pose").c_evaluator(), tiny_gen(g, "blink").c_evaluator()
    Tn = 20
    audio, z = T_(g["pose:T20:audio"])[0].cuda(), T_(g["pose:T20:z"])[:, 0].contiguous().cuda()
    x0 = T_(g["pose:T20:init"])[0, 0].cuda()
    out, outb = torch.full((Tn, 6), float("nan"), device="cuda"), torch.full((Tn, 2), float("nan"), device="cuda")
    need = evp.workspace_bytes(Tn)
    sneed = int(L.dawn_pose_blink_workspace_bytes(evp.h, evb.h, Tn))
    ws = torch.zeros(sneed, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: L.dawn_last_error().decode()                                              # noqa: E731

    def gen_call(z_ptr, T, nbytes):
        return L.dawn_pbnet_generate(evp.h, x0.data_ptr(), audio.data_ptr(), 48, z_ptr, T, out.data_ptr(), 6, ws.data_ptr(), nbytes, st)
    assert gen_call(z.data_ptr(), Tn, need - 1) != 0 and "workspace" in err()
    assert gen_call(z.data_ptr(), 0, need) != 0 and "T = 0" in err()
    assert gen_call(None, Tn, need) != 0 and "NULL" in err()
    assert L.dawn_pbnet_generate(evp.h, x0.data_ptr(), audio.data_ptr(), 48, z.data_ptr(), Tn, ws.data_ptr() + 1024, 6, ws.data_ptr(), need,
                                 st) != 0 and "overlaps" in err()
    ip, ib = (C.c_float * 6)(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), (C.c_float * 2)(0.3, 0.28)

    def stage_call(zb_ptr, T, nbytes):
        return L.dawn_pose_blink_stage(evp.h, evb.h, audio.data_ptr(), 48, T, ip, ib, z.data_ptr(), zb_ptr, out.data_ptr(), 6, outb.data_ptr(),
                                       2, ws.data_ptr(), nbytes, st)
    assert stage_call(z.data_ptr(), Tn, sneed - 1) != 0 and "workspace" in err()            # both decoders are checked before the first launch
    assert stage_call(z.data_ptr(), 0, sneed) != 0 and "T = 0" in err()
    assert stage_call(None, Tn, sneed) != 0 and "NULL" in err()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(outb).all())
    assert gen_call(z.data_ptr(), Tn, need) == 0                            # the same arguments, whole: accepted
    torch.cuda.synchronize()
    check("pbnet_via_c/raw_call", out, T_(g["pose:T20:out"])[0], 2e-5)
