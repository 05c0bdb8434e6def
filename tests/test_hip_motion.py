"""-m gpu: the LFG motion encode on the device (csrc/motion_encode.hip, motion_encoder.py, FlowDiffusion.encode_video / reenact).

Each of the five kernels runs from the reference's own upstream values (the stage goldens of tools/gen_goldens_motion.py; inputs that are
not stored come from tests/motion_cases.frames_u8) and is held to the project tolerance 1e-4 * max(1, |y|) against the reference's fp32
result, and to the float64 gate of motion_cases.assert_gate: kernel error against the float64 restatement <= 5 x the error of the
reference's own fp32 result against the same float64, both printed.  `affine` is checked as A A^T = covar and through M = A_s inverse(A_d)
after the sign fix, at the tolerance divided by the relative eigen-gap (motion_cases.check_motion_matrices).  End to end: encode_clip on
cases A and B, a chunked run bit-identical to the unchunked one, encode_video's decoded frames, reenact's bytes, and the five entries
between guard bands.

Measured on an MI355X (ratio kernel-vs-fp64 / reference-fp32-vs-fp64, gate 5): antialias_down 1.4, shift 0.32, covar 0.23, bg_params 1.0,
motion_inputs 0.94, flow 1.0, occlusion 1.04; M at 0.14 % of its eigen-gap bound; profiles/motion_encode.md has the errors themselves."""
import pytest
import torch

import motion_cases as mc
from guarded import GuardedOps

pytestmark = pytest.mark.gpu
R, S = mc.R, mc.S


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def sds():
    return mc.state_dicts()


@pytest.fixture(scope="module")
def gA():
    return mc.golden("A")


@pytest.fixture(scope="module")
def gB():
    return mc.golden("B")


@pytest.fixture(scope="module")
def encoder(hip, sds):
    from dawn_pytorch_amd.motion_encoder import MotionEncoder
    return MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cuda", ops=hip)


def cuda(p):
    return tuple(t.cuda().contiguous() for t in p)


def frames(case):
    src_u8, drv_u8 = mc.frames_u8(case)
    return torch.from_numpy(src_u8), torch.from_numpy(drv_u8), mc.to_float(src_u8), mc.to_float(drv_u8)


# ---------------------------------------------------------------------------------------------- the five kernels from their golden inputs
def test_antialias_down_fp32_and_bytes(hip, gA, gB):
    for name, g in (("A", gA), ("B", gB)):
        c = mc.CASES[name]
        h, w = c["H"] // S, c["W"] // S
        src_u8, drv_u8, src, drv = frames(name)
        x = torch.cat((src.unsqueeze(0), drv), 0)
        want64 = mc.antialias_down(x, S)
        want32 = torch.cat((g["down_src"].unsqueeze(0), g["down_drv"]), 0) if "down_drv" in g else g["down_src"].unsqueeze(0)
        n = want32.shape[0]
        got = hip.antialias_down(x.cuda(), S, 16)
        assert got.shape == ((c["T"] + 1) * h * w, 16) and not bool(got[:, 3:].any())
        got = mc.maps_of(got[:, :3], c["T"] + 1, h, w).cpu()
        mc.assert_close(got[:n], want32, f"{name} antialias_down")
        mc.assert_gate(got[:n], want32, want64[:n], f"{name} antialias_down gate")
        mc.assert_close(got, want64, f"{name} antialias_down, every frame vs fp64")
        # the same frames as bytes, and as a (3,T,H,W) clip permuted (frame stride < channel stride)
        u8 = hip.antialias_down(torch.cat((src_u8.unsqueeze(0), drv_u8), 0).cuda(), S, 16)
        assert torch.equal(mc.maps_of(u8[:, :3], c["T"] + 1, h, w).cpu(), got)
        clip = x.permute(1, 0, 2, 3).contiguous().cuda()
        assert torch.equal(hip.antialias_down(clip.permute(1, 0, 2, 3), S, 16)[:, :3].cpu(), u8[:, :3].cpu())
    # scale 1: the layout change alone, exact
    one = hip.antialias_down(drv.cuda(), 1, 16)
    assert torch.equal(one[:, :3].cpu(), mc.rows_of(drv)) and not bool(one[:, 3:].any())


@pytest.mark.parametrize("name", ["A", "B"])
def test_region_moments(hip, gA, gB, name):
    g = gA if name == "A" else gB
    c = mc.CASES[name]
    T, h, w = c["T"], c["H"] // S, c["W"] // S
    x = g["drv_regions"]
    shift, covar, affine = hip.region_moments(mc.rows_of(x).cuda(), T, h, w, R, mc.TEMPERATURE)
    s64, c64, _ = mc.region_moments(x.reshape(T, R, h * w).transpose(1, 2), h, w)
    mc.assert_close(shift, g["drv_shift"], f"{name} shift")
    mc.assert_close(covar, g["drv_covar"], f"{name} covar")
    mc.assert_gate(shift, g["drv_shift"], s64, f"{name} shift gate")
    mc.assert_gate(covar, g["drv_covar"], c64, f"{name} covar gate")
    mc.check_affine(affine, g["drv_covar"], f"{name} affine")
    assert bool((torch.det(affine.double().cpu()) < 0).all())                               # det U = -1: the header's convention
    if "src_regions" in g:
        s_shift, s_covar, s_aff = hip.region_moments(mc.rows_of(g["src_regions"]).cuda(), 1, h, w, R, mc.TEMPERATURE)
        mc.assert_close(s_shift[0], g["src_shift"], f"{name} source shift")
        mc.assert_close(s_covar[0], g["src_covar"], f"{name} source covar")
        mc.check_affine(s_aff[0], g["src_covar"], f"{name} source affine")
        mc.check_motion_matrices(s_aff, affine, (g["src_covar"], g["src_affine"], g["src_u"]), (g["drv_covar"], g["drv_affine"], g["drv_u"]),
                                 f"{name} M = A_s inverse(A_d), source against every frame")
    # the golden's driving frames against each other: frame 0 as the `source` of the later ones
    mc.check_motion_matrices(affine[:1], affine[1:], (g["drv_covar"][:1], g["drv_affine"][:1], g["drv_u"][:1]),
                             (g["drv_covar"][1:], g["drv_affine"][1:], g["drv_u"][1:]), f"{name} M, frame 0 against the later frames")


def test_region_moments_row_stride_and_exact_diagonal(hip):
    """A 16-wide row buffer whose columns past R hold NaN; a symmetric map: covar is diagonal up to rounding and U stays a reflection."""
    h = w = 9
    yy, xx = torch.meshgrid(torch.arange(h).float() - 4, torch.arange(w).float() - 4, indexing="ij")
    x = torch.full((h * w, 16), float("nan"))
    for r in range(R):
        x[:, r] = (-(xx * xx) / (2.0 + r) - (yy * yy) / (1.0 + 0.5 * r)).reshape(-1) * 0.02
    shift, covar, affine = hip.region_moments(x.cuda(), 1, h, w, R, mc.TEMPERATURE)
    s64, c64, a64 = mc.region_moments(x[:, :R].unsqueeze(0), h, w)
    mc.assert_close(shift, s64, "symmetric map shift")
    mc.assert_close(covar, c64, "symmetric map covar")
    mc.check_affine(affine, c64, "symmetric map affine")
    assert bool(torch.isfinite(affine).all()) and bool((torch.det(affine.double().cpu()) < 0).all())


def test_bg_params(hip, gA, sds):
    T = mc.CASES["A"]["T"]
    last = gA["bg_last"]                                                                    # (T, C, 12, 12)
    fc_w, fc_b = sds["bg_predictor"]["fc.weight"], sds["bg_predictor"]["fc.bias"]
    got = hip.bg_params(mc.rows_of(last).cuda(), T, fc_w.cuda(), fc_b.cuda())
    mc.assert_close(got, gA["bg_params"], "bg_params")
    mc.assert_gate(got, gA["bg_params"], mc.bg_params(last.flatten(2).transpose(1, 2), fc_w, fc_b), "bg_params gate")


def test_motion_inputs(hip, gA):
    T, h, w = mc.CASES["A"]["T"], 24, 24
    drv, src = mc.region_params(gA, "drv"), mc.region_params(gA, "src")
    src_rows = torch.zeros(h * w, 16)
    src_rows[:, :3] = mc.rows_of(gA["down_src"].unsqueeze(0))
    got = hip.motion_inputs(cuda(drv), cuda(src), gA["bg_params"].cuda(), src_rows.cuda(), T, h, w, 48)
    assert got.shape == (T * h * w, 48) and not bool(got[:, 44:].any())
    got = mc.maps_of(got[:, :44], T, h, w).cpu()
    want64 = mc.motion_inputs(drv, src, gA["bg_params"], gA["down_src"])
    fr = gA["pf_in_frames"].tolist()
    mc.assert_close(got[fr], gA["pf_in"], "motion_inputs")
    mc.assert_gate(got[fr], gA["pf_in"], want64[fr], "motion_inputs gate")
    mc.assert_close(got, want64, "motion_inputs, every frame vs fp64")


def test_flow_combine_both_conf_conventions(hip, gA):
    T, h, w = mc.CASES["A"]["T"], 24, 24
    drv, src = cuda(mc.region_params(gA, "drv")), cuda(mc.region_params(gA, "src"))
    x = torch.zeros(T * h * w, 16)
    x[:, :12] = mc.rows_of(gA["mask_occ"])
    lat = torch.full((3, T + 2, h, w), float("nan"), device="cuda")                         # a frame range of a longer (3,Ttot,h,w) latent
    conf = torch.empty(T, h, w, device="cuda")
    hip.flow_combine(x.cuda(), drv, src, gA["bg_params"].cuda(), T, h, w, lat[:2, 1:T + 1], conf)
    flow64, occ64 = mc.flow_combine(gA["mask_occ"], mc.region_params(gA, "drv"), mc.region_params(gA, "src"), gA["bg_params"])
    got = lat[:2, 1:T + 1].permute(1, 2, 3, 0).cpu()
    mc.assert_close(got, gA["optical_flow"], "flow_combine flow")
    mc.assert_gate(got, gA["optical_flow"], flow64, "flow_combine flow gate")
    mc.assert_close(conf.unsqueeze(1), gA["occlusion_map"], "flow_combine occlusion")
    mc.assert_gate(conf.unsqueeze(1), gA["occlusion_map"], occ64, "flow_combine occlusion gate")
    assert bool(torch.isnan(lat[:, 0]).all()) and bool(torch.isnan(lat[:, T + 1]).all()) and bool(torch.isnan(lat[2]).all())
    x0 = torch.empty(T, h, w, device="cuda")
    hip.flow_combine(x.cuda(), drv, src, gA["bg_params"].cuda(), T, h, w, lat[:2, 1:T + 1], x0, conf_x0=True)
    assert torch.equal(x0, 2.0 * conf - 1.0)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["A", "B"])
def test_encode_clip_matches_the_reference(encoder, gA, gB, name):
    g = gA if name == "A" else gB
    c = mc.CASES[name]
    T, h, w = c["T"], c["H"] // S, c["W"] // S
    _, drv_u8, src, drv = frames(name)
    out = encoder.encode_clip(src.cuda(), drv.cuda())
    assert out["real_vid_grid"].shape == (1, 2, T, h, w) and out["real_vid_conf"].shape == (1, 1, T, h, w)
    mc.assert_close(out["real_vid_grid"][0].permute(1, 2, 3, 0), g["optical_flow"], f"{name} encode_clip optical_flow")
    mc.assert_close(out["real_vid_conf"][0, 0].unsqueeze(1), g["occlusion_map"], f"{name} encode_clip occlusion_map")
    lat = encoder.latent(src.cuda(), drv_u8.cuda())                                         # bytes in, the x0 convention out
    assert torch.equal(lat[:2], out["real_vid_grid"][0]) and torch.equal(lat[2], 2.0 * out["real_vid_conf"][0, 0] - 1.0)


def test_chunked_run_is_bit_identical(encoder):
    _, _, src, drv = frames("A")
    whole = encoder.encode_clip(src.cuda(), drv.cuda(), chunk=5)
    parts = encoder.encode_clip(src.cuda(), drv.cuda(), chunk=2)
    assert torch.equal(whole["real_vid_grid"], parts["real_vid_grid"]) and torch.equal(whole["real_vid_conf"], parts["real_vid_conf"])


@pytest.fixture(scope="module")
def flow_diffusion(encoder, sds):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    dec = FlowDecoder(sds["generator"], "cuda")
    return FlowDiffusion(img_size=24, num_frames=5, generator=dec, motion_encoder=encoder, device="cuda")


def test_encode_video_decodes_the_reference_prediction(flow_diffusion, gA):
    T = mc.CASES["A"]["T"]
    _, _, src, drv = frames("A")
    out = flow_diffusion.encode_video(src.unsqueeze(0).cuda(), drv.permute(1, 0, 2, 3).unsqueeze(0).cuda())
    assert set(out) == {"real_vid_grid", "real_vid_conf", "real_out_vid", "real_warped_vid"}
    assert out["real_out_vid"].shape == (1, 3, T, 96, 96)
    fr = gA["prediction_frames"].tolist()
    mc.assert_close(out["real_out_vid"][0, :, fr].permute(1, 0, 2, 3), gA["prediction"], "encode_video real_out_vid")
    mc.assert_close(out["real_warped_vid"][0, :, fr].permute(1, 0, 2, 3), gA["deformed"], "encode_video real_warped_vid")


def test_reenact_bytes_equal_decode_of_the_encoded_latent(flow_diffusion, encoder):
    import numpy as np
    _, drv_u8, src, drv = frames("A")
    img = src.unsqueeze(0).cuda()
    enc = encoder.encode_clip(src.cuda(), drv.cuda())
    dec = flow_diffusion.flow_decoder("cuda")
    want = dec.decode_clip_u8(img, enc["real_vid_grid"], enc["real_vid_conf"])
    out = flow_diffusion.reenact(img, drv.permute(1, 0, 2, 3).unsqueeze(0).cuda(), frames_u8=dict())
    assert torch.equal(out["sample_frames_u8"], want) and torch.equal(out["real_vid_grid"], enc["real_vid_grid"])
    # bytes in, yuv420p out, streamed in chunks of 2
    yuv = dec.decode_clip_yuv420(img, enc["real_vid_grid"], enc["real_vid_conf"])
    got = flow_diffusion.reenact(img, drv_u8.cuda(), frames_u8=dict(format="yuv420p", stream=True, chunk=2))
    chunks = [(t0, fr.copy()) for t0, fr in got["sample_frames_yuv420"]]
    assert [t0 for t0, _ in chunks] == [0, 2, 4]
    assert np.array_equal(np.concatenate([fr for _, fr in chunks], 0), yuv[0].cpu().numpy())
    fp32 = flow_diffusion.reenact(img, drv.permute(1, 0, 2, 3).unsqueeze(0).cuda())
    assert fp32["sample_out_vid"].shape == (1, 3, 5, 96, 96)


# ---------------------------------------------------------------------------------------------- guard bands and poison
def test_five_entries_between_guard_bands(gA, sds):
    T, h, w = mc.CASES["A"]["T"], 24, 24
    g = GuardedOps()
    _, drv_u8, _, drv = frames("A")
    frames_in, _ = g.guarded_in(drv.reshape(T * 3, 96 * 96), name="frames")
    down = g.antialias_down(frames_in.view(T, 3, 96, 96), S, 16)
    bytes_in, _ = g.guarded_in(drv_u8.reshape(T, -1), name="bytes")
    down_u8 = g.antialias_down(bytes_in.view(T, 96, 96, 3), S, 16)
    x_in, _ = g.guarded_in(mc.rows_of(gA["drv_regions"]), name="regions")
    moments = g.region_moments(x_in, T, h, w, R, mc.TEMPERATURE)
    last_in, _ = g.guarded_in(mc.rows_of(gA["bg_last"]), name="bg_last")
    bg = g.bg_params(last_in, T, sds["bg_predictor"]["fc.weight"].cuda(), sds["bg_predictor"]["fc.bias"].cuda())
    drv_p = tuple(g.guarded_in(t.reshape(T * R, -1), name=f"drv{i}")[0].view(t.shape) for i, t in enumerate(mc.region_params(gA, "drv")))
    src_p = tuple(g.guarded_in(t.reshape(R, -1), name=f"src{i}")[0].view(t.shape) for i, t in enumerate(mc.region_params(gA, "src")))
    bg_in = g.guarded_in(gA["bg_params"].reshape(T, 9), name="bg")[0].view(T, 3, 3)
    src_rows = torch.zeros(h * w, 16)
    src_rows[:, :3] = mc.rows_of(gA["down_src"].unsqueeze(0))
    rows_in, _ = g.guarded_in(src_rows, name="src_rows")
    rows = g.motion_inputs(drv_p, src_p, bg_in, rows_in, T, h, w, 48)
    x = torch.zeros(T * h * w, 16)
    x[:, :12] = mc.rows_of(gA["mask_occ"])
    mo_in, _ = g.guarded_in(x, name="mask_occ")
    grid = g.guarded_out(2 * T, h * w, name="grid").view(2, T, h, w)
    conf = g.guarded_out(T, h * w, name="conf").view(T, h, w)
    g.flow_combine(mo_in, drv_p, src_p, bg_in, T, h, w, grid, conf)
    torch.cuda.synchronize()
    g.verify()
    g.inputs_intact()
    names = {r.name for r in g.outs}
    assert {"antialias_down.out", "region_moments.shift", "region_moments.covar", "region_moments.affine", "bg_params.out",
            "motion_inputs.out", "grid", "conf"} <= names, names
    assert torch.equal(down, down_u8) and bool(torch.isfinite(rows).all()) and bool(torch.isfinite(bg).all())
    mc.assert_close(moments[0], gA["drv_shift"], "guarded shift")
    mc.assert_close(grid.permute(1, 2, 3, 0), gA["optical_flow"], "guarded flow")
