"""-m gpu: the motion-encode stage from C (csrc/dawn_motion.hip: dawn_motion_*, dawn_reenact_*), the yuv420p ingest in front of it
(csrc/yuv_ingest.hip: dawn_yuv420_to_frames), its bundle stage and the program's --driving mode.

* The converter, byte for byte against the integer restatement of tests/yuv_cases.py: one 4096 x 4096 frame that holds every (Y, U, V)
  triple once; the smallest shape, a padded frame stride, rows that are no multiple of the wide block, a wide-path clip with a padded
  stride, a stride and a pointer that force the narrow path at W % 8 == 0; between guard bands; its refusals.
* The stage against the Python orchestration (`MotionEncoder.encode_clip`, same chunk): `torch.equal`.  EVERY launch of the Python path is
  issued with the same arguments; the one launch Python does not have is the copy kernel that repeats the source half of the background
  encoder's first conv for the frames of a chunk (Python: expand().reshape(), a torch copy) -- it moves bits and changes no arithmetic, so
  no output is held to anything weaker than equality.
* The stage against the reference goldens at the existing tolerance (motion_cases.assert_close: 1e-4 max(1, |y|)).
* Chunking and input kinds, reenactment in one call against `FlowDiffusion.reenact`, the bundle stage, a workspace of exactly the
  queried size between guard bands with the outputs as slices of a NaN-filled latent, the refusals, and tools/dawn_generate.cpp
  --driving as a fresh child process."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import motion_cases as mc
import yuv_cases as yc
from conftest import ROOT
from guarded import GuardedOps, assert_no_255
from test_hip_clip_inputs import hip, stages  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
R, S = mc.R, mc.S
MEAN = (2.0, 0.0, -3.5)


def lib():
    from dawn_pytorch_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- the converter
def convert(hip, frames, H, W):  # noqa: F811
    return hip.yuv420_to_frames(torch.from_numpy(frames).cuda(), H, W).cpu().numpy()


def test_converter_exhaustive(hip):  # noqa: F811
    """Every (Y, U, V) triple once, 4096 x 4096 (the wide path); compared on the device against the uploaded expectation."""
    frame = yc.exhaustive_frame()
    want = torch.from_numpy(yc.frames_to_rgb(frame, 4096, 4096)).cuda()
    got = hip.yuv420_to_frames(torch.from_numpy(frame).cuda(), 4096, 4096)
    assert got.shape == (1, 4096, 4096, 3) and torch.equal(got, want)


@pytest.mark.parametrize("T,H,W,extra,offset", [(1, 2, 4, 0, 0), (3, 6, 12, 20, 0), (2, 96, 100, 0, 0), (2, 4, 16, 8, 0), (2, 4, 16, 4, 0), (2, 4, 16, 0, 1),
                                                (3, 10, 24, 0, 0)],
                         ids=["smallest", "padded-stride", "w100", "wide-padded", "wide-shape-odd-stride", "wide-shape-odd-pointer", "wide-odd-rows"])
def test_converter_shapes(hip, T, H, W, extra, offset):  # noqa: F811
    n = H * W * 3 // 2
    frames = yc.random_frames(T, H, W, stride=n + extra, seed=T * 1000 + W)
    want = yc.frames_to_rgb(frames, H, W)
    dev = torch.full((T * (n + extra) + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    view = dev[offset:offset + T * (n + extra)].view(T, n + extra)
    view.copy_(torch.from_numpy(frames))
    got = hip.yuv420_to_frames(view, H, W)
    assert np.array_equal(got.cpu().numpy(), want)
    other = frames.copy()
    other[:, n:] = 0x11                                            # the padding between frames is never read
    assert np.array_equal(convert(hip, other, H, W), want)


def test_converter_between_guard_bands_and_refusals():
    g = GuardedOps()
    L = g.L
    for T, H, W in ((2, 6, 12), (2, 8, 32)):                      # the narrow and the wide kernel
        n = H * W * 3 // 2
        rng = np.random.default_rng(W)
        frames = np.concatenate((rng.integers(16, 181, (T, H * W), dtype=np.uint8), rng.integers(100, 157, (T, n - H * W), dtype=np.uint8)), 1)
        want = yc.frames_to_rgb(frames, H, W)
        assert_no_255(want)                                        # 255 is the poison of a byte payload (tests/guarded.py)
        src, _ = g.guarded_in(torch.from_numpy(frames), name=f"yuv{W}")
        out = g.guarded_out(T, H * W * 3, name=f"rgb{W}", dtype=torch.uint8)
        g.yuv420_to_frames(src, H, W, out=out.view(T, H, W, 3))
        torch.cuda.synchronize()
        g.verify()
        g.inputs_intact()
        assert np.array_equal(out.view(T, H, W, 3).cpu().numpy(), want)
    # refusals: the argument named, nothing launched -- the poisoned output is untouched
    src = torch.zeros(4 * 64, dtype=torch.uint8, device="cuda")
    out = g.guarded_out(1, 4 * 64, name="untouched", dtype=torch.uint8)
    p, o = src.data_ptr(), out.data_ptr()
    for args, name in (((p, 18, 1, 3, 4, o), "H = 3"), ((p, 18, 1, 2, 6, o), "W = 6"), ((None, 12, 1, 2, 4, o), "in is NULL"),
                       ((p, 12, 1, 2, 4, None), "out is NULL"), ((p, 11, 1, 2, 4, o), "frame_stride = 11"), ((p, 12, 1, 2, 4, o + 2), "out is not 4-byte aligned")):
        assert L.dawn_yuv420_to_frames(*args, stream()) != 0 and name in L.dawn_last_error().decode(), name
    torch.cuda.synchronize()
    for r in g.outs:
        r.check_surroundings("write outside the buffer")
    assert bool((out == 255).all())


# ---------------------------------------------------------------------------------------------- the stage
@pytest.fixture(scope="module")
def sds():
    return mc.state_dicts()


@pytest.fixture(scope="module")
def encoder(hip, sds):  # noqa: F811
    from dawn_pytorch_amd.motion_encoder import MotionEncoder
    return MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cuda", ops=hip)


@pytest.fixture(scope="module")
def ev(encoder):
    from dawn_pytorch_amd.ctx import MotionEvaluator
    return MotionEvaluator(encoder)


@pytest.fixture(scope="module")
def decoder(hip, sds):  # noqa: F811
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    return FlowDecoder(sds["generator"], "cuda", ops=hip)


@pytest.fixture(scope="module")
def dec_ev(decoder):
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    return DecoderEvaluator(decoder)


def frames(case):
    src_u8, drv_u8 = mc.frames_u8(case)
    return torch.from_numpy(src_u8), torch.from_numpy(drv_u8), mc.to_float(src_u8).cuda(), mc.to_float(drv_u8).cuda()


@pytest.fixture(scope="module")
def python_path(encoder):
    """MotionEncoder.encode_clip of cases A and B at the default chunk: computed once, shared, never modified."""
    out = {}
    for case in ("A", "B"):
        _, _, src, drv = frames(case)
        out[case] = encoder.encode_clip(src, drv)
    return out


@pytest.mark.parametrize("case", ["A", "B"])
def test_stage_equals_the_python_path_and_meets_the_goldens(ev, encoder, python_path, case):
    """Items 4 and 5.  The launches and their arguments are the Python path's; the one extra launch (the copy that repeats the source rows
    of the background encoder's first conv, where Python calls expand().reshape()) changes no arithmetic: equality throughout."""
    c = mc.CASES[case]
    T, h, w = c["T"], c["H"] // S, c["W"] // S
    _, _, src, drv = frames(case)
    want = python_path[case]
    got = ev.encode_clip(src, drv)
    assert got["real_vid_grid"].shape == (1, 2, T, h, w) and got["real_vid_conf"].shape == (1, 1, T, h, w)
    assert torch.equal(got["real_vid_grid"], want["real_vid_grid"]) and torch.equal(got["real_vid_conf"], want["real_vid_conf"])
    via = encoder.encode_clip(src, drv, via_c=True)                                         # the public switch
    assert torch.equal(via["real_vid_grid"], want["real_vid_grid"]) and torch.equal(via["real_vid_conf"], want["real_vid_conf"])
    g = mc.golden(case)
    mc.assert_close(got["real_vid_grid"][0].permute(1, 2, 3, 0), g["optical_flow"], f"{case} C stage optical_flow")
    mc.assert_close(got["real_vid_conf"][0, 0].unsqueeze(1), g["occlusion_map"], f"{case} C stage occlusion_map")
    if case == "A":                                                                         # a chunk that leaves a ragged last one, both hosts
        p2 = encoder.encode_clip(src, drv, chunk=2)
        c2 = ev.encode_clip(src, drv, chunk=2)
        assert torch.equal(c2["real_vid_grid"], p2["real_vid_grid"]) and torch.equal(c2["real_vid_conf"], p2["real_vid_conf"])


@pytest.fixture(scope="module")
def i420(hip):  # noqa: F811
    """Case A's driving frames as I420 bytes (the project's own egress), and what the converter makes of them."""
    _, _, _, drv = frames("A")
    yuv = hip.frames_to_yuv420(drv.permute(1, 0, 2, 3).contiguous())
    return yuv, hip.yuv420_to_frames(yuv, 96, 96)


def test_chunking_and_input_kinds(ev, encoder, python_path, i420):
    from dawn_pytorch_amd import _lib
    T, H, W, h, w = 5, 96, 96, 24, 24
    _, drv_u8, src, drv = frames("A")
    want = python_path["A"]

    def same(a, b):
        return torch.equal(a["real_vid_grid"], b["real_vid_grid"]) and torch.equal(a["real_vid_conf"], b["real_vid_conf"])
    for chunk in (1, 2, 5):
        assert same(ev.encode_clip(src, drv, chunk=chunk), want), chunk
    assert same(ev.encode_clip(src, drv_u8.cuda()), want)                                   # uint8 RGB frames: the same bits as byte / 255 planes
    assert same(ev.encode_clip(src, drv.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)), want)      # a (3,T,H,W) clip permuted, no copy
    src_u8 = torch.from_numpy(mc.frames_u8("A")[0]).unsqueeze(0).cuda()
    assert same(ev.encode_clip(src_u8, drv_u8.cuda()), want)                                # the source as bytes too
    yuv, rgb = i420
    k1 = ev.encode_clip(src, rgb, chunk=2)
    assert same(ev.encode_clip(src, yuv, chunk=2), k1) and same(encoder.encode_clip(src, rgb, chunk=2), k1)
    padded = torch.full((T, yuv.shape[1] + 20), 0x5A, dtype=torch.uint8, device="cuda")    # a frame stride above the frame
    padded[:, :yuv.shape[1]] = yuv
    assert same(ev.encode_clip(src, padded[:, :yuv.shape[1]], chunk=2), k1)
    assert same(encoder.encode_clip(src, yuv, chunk=2, via_c=True), k1)
    # conf_x0: 2 * conf - 1, within one rounding of the conf_x0 = 0 run
    lat = ev.latent(src, drv)
    assert torch.equal(lat[:2], want["real_vid_grid"][0])
    ref = 2.0 * want["real_vid_conf"][0, 0].double() - 1.0
    assert bool(((lat[2].double() - ref).abs() <= 2.0 ** -24 * ref.abs().clamp(min=2.0 ** -126)).all())
    assert torch.equal(lat, encoder.latent(src, drv))
    # the workspace does not depend on the clip length: the query has no T, and clips of 5 and of 500 frames encode in the same bytes
    assert len(_lib.SIGNATURES["dawn_motion_workspace_bytes"]) == 4
    ws = torch.empty(ev.workspace_bytes(H, W, 2), dtype=torch.uint8, device="cuda")
    long = drv_u8.repeat(100, 1, 1, 1).cuda()
    out = ev.encode_clip(src, long, chunk=2, workspace=ws)
    short = ev.encode_clip(src, drv_u8.cuda(), chunk=2, workspace=ws)
    assert torch.equal(out["real_vid_grid"][:, :, 495:], short["real_vid_grid"]) and same(short, want)
    assert ev.workspace_bytes(H, W, 2) < ev.workspace_bytes(H, W, 4) < ev.workspace_bytes(H, W, 8)


@pytest.fixture(scope="module")
def reenacted(encoder, decoder, i420):
    """Item 7's expectation, from the Python path: FlowDiffusion.reenact on case A (driving = the converted I420 frames), RGB and yuv420p."""
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    fd = FlowDiffusion(img_size=24, num_frames=5, generator=decoder, motion_encoder=encoder, device="cuda")
    _, _, src, _ = frames("A")
    img = src.unsqueeze(0)
    rgb = fd.reenact(img, i420[1], frames_u8=dict(mean=MEAN))
    yuv = fd.reenact(img, i420[1], frames_u8=dict(format="yuv420p", mean=MEAN))
    return dict(fd=fd, rgb=rgb["sample_frames_u8"][0], yuv=yuv["sample_frames_yuv420"][0], grid=rgb["real_vid_grid"], conf=rgb["real_vid_conf"])


def test_reenact_in_one_call(ev, dec_ev, reenacted, i420):
    _, _, src, _ = frames("A")
    yuv_in, rgb_in = i420
    for drv in (rgb_in, yuv_in):                                                             # kind 1 and kind 2 driving frames
        got, grid, conf = ev.reenact(dec_ev, src, drv, mean=MEAN, want_motion=True)
        assert got.shape == (5, 96, 96, 3) and torch.equal(got, reenacted["rgb"])
        assert torch.equal(grid, reenacted["grid"][0]) and torch.equal(conf, reenacted["conf"][0, 0])
        got = ev.reenact(dec_ev, src, drv, format="yuv420p", mean=MEAN, motion_chunk=2, chunk=2)
        assert got.shape == (5, 96 * 96 * 3 // 2) and torch.equal(got, reenacted["yuv"])
    # FlowDiffusion.motion_via_c: the same bytes, and I420 driving frames are taken
    fd = reenacted["fd"]
    fd.motion_via_c = True
    try:
        out = fd.reenact(src.unsqueeze(0), yuv_in, frames_u8=dict(mean=MEAN))
        assert torch.equal(out["sample_frames_u8"][0], reenacted["rgb"]) and torch.equal(out["real_vid_grid"], reenacted["grid"])
    finally:
        fd.motion_via_c = False
    with pytest.raises(ValueError, match="motion_via_c"):
        fd.reenact(src.unsqueeze(0), yuv_in, frames_u8=dict())
    # the size query's sum rule, and a workspace one byte short
    from dawn_pytorch_amd import ctx
    a = ctx.ReenactArgs()
    a.size, a.motion, a.decoder, a.img3, a.H, a.W = C.sizeof(a), ev.h, dec_ev.h, src.data_ptr(), 96, 96
    a.drv, a.drv_kind, a.T, a.drv_frame_stride, a.motion_chunk, a.chunk, a.format = yuv_in.data_ptr(), 2, 5, yuv_in.shape[1], 2, 5, 1
    cb, wb = C.c_size_t(0), C.c_size_t(0)
    L = lib()
    assert L.dawn_reenact_bytes(C.addressof(a), C.byref(cb), C.byref(wb)) == 0, L.dawn_last_error().decode()
    up = lambda n: (n + 255) // 256 * 256                                                  # noqa: E731
    skip = int(L.dawn_decoder_skip_bytes(dec_ev.h, 96, 96))
    assert cb.value == 5 * 96 * 96 * 3 // 2
    assert wb.value == up(2 * 5 * 24 * 24 * 4) + up(5 * 24 * 24 * 4) + up(skip) + max(ev.workspace_bytes(96, 96, 2), dec_ev.workspace_bytes(96, 96, 5))
    out = torch.full((cb.value,), 255, dtype=torch.uint8, device="cuda")
    ws = torch.empty(wb.value, dtype=torch.uint8, device="cuda")
    a.frames_out = out.data_ptr()
    assert L.dawn_reenact_clip(C.addressof(a), ws.data_ptr(), wb.value - 1, stream()) != 0
    assert f"workspace of {wb.value - 1} bytes, {wb.value} needed (dawn_reenact_bytes)" in L.dawn_last_error().decode()
    a.size -= 8
    assert L.dawn_reenact_clip(C.addressof(a), ws.data_ptr(), wb.value, stream()) != 0 and "args->size" in L.dawn_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 255).all())


# ---------------------------------------------------------------------------------------------- the bundle
@pytest.fixture(scope="module")
def model(stages, encoder, dec_ev, tmp_path_factory):  # noqa: F811
    """The tiny five-stage pipeline of tests/test_hip_clip_inputs.py with case A's decoder in the decoder's place (96 x 96), plus the motion
    stage; and the same without it."""
    from dawn_pytorch_amd import bundle, ctx
    e = stages["ev"]
    pipe = ctx.PipelineEvaluator(e["hub"], e["pose"], e["blink"], dec_ev, e["inp"], e["unet"])
    d = tmp_path_factory.mktemp("motion_model")
    steps = {f"ddim.{len(stages['steps'])}": stages["steps"]}
    defaults = dict(H=96, max_n_frames=8, mean=MEAN)
    with_motion, without = str(d / "motion.dawn"), str(d / "plain.dawn")
    idx = bundle.bundle_from_pipeline(with_motion, pipe, steps, defaults, motion=encoder)
    bundle.bundle_from_pipeline(without, pipe, steps, defaults)
    return dict(path=with_motion, plain=without, index=idx)


def test_bundle_motion_stage(model, encoder, python_path):
    from dawn_pytorch_amd import _lib, ctx
    stage = [e for e in model["index"]["entries"] if e["stage"] == "motion"]
    table = ctx.motion_named_weights(encoder)
    assert {e["name"] for e in stage if e["kind"] == 0} == set(table) and [e["name"] for e in stage if e["kind"] == 1] == ["cfg"]
    be = ctx.BundleEvaluator(model["path"])                                                 # open, upload, dawn_bundle_verify, the six handles
    be.verify()
    assert bytes(be.cfg(7, ctx.MotionCfg)) == bytes(ctx.motion_cfg(encoder)) and set(be.table(7)) == set(table)
    for name, t in table.items():
        raw = t.contiguous().reshape(-1).view(torch.uint8)
        assert torch.equal(be.tensor("motion", name)[:raw.numel()], raw), name
    mev = be.motion()
    _, _, src, drv = frames("A")
    got = mev.encode_clip(src, drv)
    assert torch.equal(got["real_vid_grid"], python_path["A"]["real_vid_grid"]) and torch.equal(got["real_vid_conf"], python_path["A"]["real_vid_conf"])
    del mev
    plain = ctx.BundleEvaluator(model["plain"])                                             # dawn_bundle_create_handles still succeeds without the stage
    assert all(s.h for s in plain.ev)
    with pytest.raises(_lib.DawnHipError, match="dawn_bundle_create_motion.*stage 'motion' is missing"):
        plain.motion()


# ---------------------------------------------------------------------------------------------- guard bands, refusals
def test_guarded_workspace_and_strided_outputs(ev, python_path):
    T, H, W, h, w = 5, 96, 96, 24, 24
    _, drv_u8, src, _ = frames("A")
    g = GuardedOps()
    need = ev.workspace_bytes(H, W, 2)
    ws = g.guarded_out(1, need, name="workspace", dtype=torch.uint8).view(-1)              # exactly the queried size, poisoned
    drv, _ = g.guarded_in(drv_u8.reshape(T, -1), name="driving")
    block = torch.full((3, T + 3, h, w), float("nan"), device="cuda")
    ev.encode_into(src, drv.view(T, H, W, 3), block[:2, 2:T + 2], block[2, 2:T + 2], chunk=2, conf_x0=True, workspace=ws)
    torch.cuda.synchronize()
    for r in g.outs:
        r.check_surroundings("write outside the workspace")
    g.inputs_intact()
    assert bool(torch.isnan(block[:, :2]).all()) and bool(torch.isnan(block[:, T + 2:]).all())
    assert not bool(torch.isnan(block[:, 2:T + 2]).any())
    assert torch.equal(block[:2, 2:T + 2], python_path["A"]["real_vid_grid"][0])
    assert torch.equal(block[2, 2:T + 2], 2.0 * python_path["A"]["real_vid_conf"][0, 0] - 1.0)


def test_refusals_name_their_cause_and_launch_nothing(ev):
    L = lib()
    T, H, W, h, w = 5, 96, 96, 24, 24
    _, drv_u8, src, _ = frames("A")
    drv = drv_u8.cuda()
    grid = torch.full((2, T, h, w), float("nan"), device="cuda")
    conf = torch.full((T, h, w), float("nan"), device="cuda")
    need = ev.workspace_bytes(H, W, 2)
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")

    def call(H=H, W=W, T=T, src_kind=0, drv_kind=1, chunk=2, bytes_=need, g=grid, s=src):
        return L.dawn_motion_encode_clip(ev.h, H, W, T, s.data_ptr() if s is not None else None, src_kind, drv.data_ptr(), drv_kind, H * W * 3, 1, chunk,
                                         g.data_ptr() if g is not None else None, T * h * w, conf.data_ptr(), 0, ws.data_ptr(), bytes_, stream())
    cases = [(dict(H=100), "must be positive multiples of 8"),                             # the background encoder pools three times
             (dict(H=40, W=40), "the 10 x 10 map"),                                        # 40 / 4 = 10: not a multiple of 8, the hourglasses refuse it
             (dict(chunk=0), "chunk = 0"), (dict(bytes_=need - 1), f"workspace of {need - 1} bytes, {need} needed (dawn_motion_workspace_bytes)"),
             (dict(drv_kind=3), "drv_kind = 3"), (dict(src_kind=2), "src_kind = 2"), (dict(T=0), "T = 0"), (dict(g=None), "grid"), (dict(s=None), "src")]
    for kw, what in cases:
        assert call(**kw) != 0, what
        msg = L.dawn_last_error().decode()
        assert "dawn_motion_encode_clip" in msg and what in msg, (what, msg)
    assert ev.workspace_bytes(100, 96, 2) == 0 and "multiples of 8" in L.dawn_last_error().decode()
    assert ev.workspace_bytes(40, 40, 2) == 0 and ev.workspace_bytes(96, 96, 0) == 0
    # I420 frames of a width the converter does not take are refused here, before the first launch: H = W = 96 is fine, a short stride is not
    assert L.dawn_motion_encode_clip(ev.h, H, W, T, src.data_ptr(), 0, drv.data_ptr(), 2, H * W * 3 // 2 - 1, 0, 2, grid.data_ptr(), T * h * w,
                                     conf.data_ptr(), 0, ws.data_ptr(), need, stream()) != 0 and "drv_frame_stride" in L.dawn_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(grid).all()) and bool(torch.isnan(conf).all()) and bool((ws == 255).all())
    # a missing weight is named, a block count beyond the struct refused
    from dawn_pytorch_amd import _lib, ctx
    table = dict(ev.weights)
    del table["pf.up.1.a"]
    with pytest.raises(_lib.DawnHipError, match="dawn_motion_create: missing packed weight 'pf.up.1.a'"):
        _create(ev.cfg, table)
    cfg = ctx.MotionCfg.from_buffer_copy(bytes(ev.cfg))
    cfg.pf_blocks = 9
    with pytest.raises(_lib.DawnHipError, match="pf_blocks = 9"):
        _create(cfg, dict(ev.weights))


def _create(cfg, table):
    """dawn_motion_create on an edited cfg / table, through the evaluators' shared base (it raises the library's message)."""
    from dawn_pytorch_amd import ctx
    return ctx._Evaluator("dawn_motion_create", "dawn_motion_destroy", cfg, table, torch.device("cuda"), fp32_only=False)


# ---------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tools/dawn_generate.cpp with the host compiler, as tests/test_hip_bundle.py builds it."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("dawn_generate_motion") / "dawn_generate")
    libdir = os.path.join(ROOT, "dawn-pytorch_amd")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                        os.path.join(ROOT, "tools", "dawn_generate.cpp"), "-L", libdir, "-ldawn_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                        f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_program_driving_mode(model, program, reenacted, i420, tmp_path):
    """One .y4m of case A's frames and one PPM of its source written here; the program runs once with --driving, a fresh child under its own
    time limit.  A child that dies of a signal or runs into the limit ends the test run at once: nothing more is started on the GPU."""
    src_u8, _ = mc.frames_u8("A")
    H, T = 96, 5
    (tmp_path / "d.y4m").write_bytes(yc.y4m_bytes(i420[0].cpu().numpy(), H, H, frame_header=b"FRAME Ip\n"))
    (tmp_path / "f.ppm").write_bytes(b"P6\n%d %d\n255\n" % (H, H) + np.ascontiguousarray(src_u8).tobytes())
    out = tmp_path / "clip.y4m"
    torch.cuda.synchronize()

    def run(bundle_path):
        try:
            r = subprocess.run([program, "--bundle", bundle_path, "--driving", str(tmp_path / "d.y4m"), "--image", str(tmp_path / "f.ppm"),
                                "--out", str(out)], capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("dawn_generate --driving ran into its time limit: no further GPU work", returncode=1)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            pytest.exit(f"dawn_generate --driving died with status {r.returncode}: no further GPU work\n{r.stderr[-2000:]}", returncode=1)
        return r
    r = run(model["path"])
    assert r.returncode == 0, r.stderr
    data = out.read_bytes()
    head = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (H, H)
    frame = H * H * 3 // 2
    assert data[:len(head)] == head and len(data) == len(head) + T * (6 + frame)
    body = data[len(head):]
    assert all(body[t * (6 + frame):][:6] == b"FRAME\n" for t in range(T))
    assert b"".join(body[t * (6 + frame) + 6:][:frame] for t in range(T)) == reenacted["yuv"].cpu().numpy().tobytes()
    # a bundle without the motion stage: the loader's message, the program's refusal status
    r = run(model["plain"])
    assert r.returncode == 3 and "stage 'motion' is missing" in r.stderr
