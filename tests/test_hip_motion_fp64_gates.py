"""-m gpu: the five kernels of the LFG motion encode (csrc/motion_encode.hip) against a float64 reference at fp32 accuracy, on the cases of
tests/motion_gate.py: non-square maps, ragged last workgroups, R = 1 and R = 15, every antialias scale and partial tiles, bg_params at the
production width, motion parameters that reach the sign fix, sign(0), regions wholly outside and a background with Z != 1.

The gate (split_gate.fp32_gate): max|hip - fp64| / max|fp64| <= c x the same for the restatement in fp32 on CPU + FLOOR, c = C_GATE = 2
unless motion_gate.C_WIDE widens it with the MI355X measurement beside it (profiles/motion_gate_ratios.md has every kernel's).
tests/test_motion_gate_cpu.py shows that every case rejects the defects of its kernel.  Each gate appends its errors and its ratio to CPU
fp32 to the op-error log.  Also: one ragged case per kernel between guard bands, dawn_motion_inputs with ld_out > c_pad from its C entry,
and the non-square golden N (96 x 128) end to end, from Python and from the C host.

Measured on an MI355X (largest GPU error / CPU fp32 error per output, gate 2): antialias_down 0.69 (2.04 before its divisor was summed in
double, which the antialias cases now also pin with motion_gate.aa_format_bound), shift 0.10, covar 0.24, bg_params 0.42, heatmap
channels 1.23, warped channels 1.01, flow 1.13, occlusion 1.00."""
import pytest
import torch

import motion_cases as mc
import motion_gate as G
from guarded import GuardedOps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def cu(p):
    return tuple(t.cuda().contiguous() for t in p) if isinstance(p, tuple) else p.cuda()


def case_named(name):
    return next(c for c in G.CASES if c.name == name)


def of_kind(kind):
    cs = [c for c in G.CASES if c.kind == kind]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def gate(case, got, T):
    """got: {output: tensor} -> every gated output through fp32_gate, logged."""
    torch.cuda.synchronize()
    want64, base32 = case.want64(T), case.base32(T)
    for o in case.gated():
        assert tuple(got[o].shape) == tuple(want64[o].shape), (case.name, o, tuple(got[o].shape), tuple(want64[o].shape))
        G.fp32_gate(f"{case.name}/{o}", got[o], want64[o], base32[o], c=case.c(o))
    return want64


# ---------------------------------------------------------------------------------------------- the calls, shared with the guarded runs
def run_aa(ops, case, x, c_pad=16):
    p = case.p
    ho, wo = case.out_hw()
    rows = ops.antialias_down(x, p["s"], c_pad)
    assert tuple(rows.shape) == (x.shape[0] * ho * wo, c_pad) and not bool(rows[:, 3:].any())          # columns 3 .. c_pad are zero
    return rows, mc.maps_of(rows[:, :3], x.shape[0], ho, wo).cpu()


def mi_maps(case, rows, T):
    p = case.p
    n = 4 * (p["R"] + 1)
    assert tuple(rows.shape) == (T * p["h"] * p["w"], p["c_pad"]) and not bool(rows[:, n:].any())       # the channels past 4 (R + 1) are zero
    return G.split_mi(mc.maps_of(rows[:, :n], T, p["h"], p["w"]).cpu())


def run_fc(ops, case, T_, rows, drv, src, bg, conf_x0):
    """Into frames 1 .. T of a NaN-filled (3, T + 2, h, w) latent; its other planes must stay NaN."""
    p, T = case.p, T_["T"]
    h, w = p["h"], p["w"]
    lat = torch.full((3, T + 2, h, w), float("nan"), device="cuda")
    conf = torch.full((T, h, w), float("nan"), device="cuda")
    ops.flow_combine(rows, drv, src, bg, T, h, w, lat[:2, 1:T + 1], conf, conf_x0=conf_x0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(lat[:, 0]).all()) and bool(torch.isnan(lat[:, T + 1]).all()) and bool(torch.isnan(lat[2]).all()), case.name
    return lat[:2, 1:T + 1].permute(1, 2, 3, 0).cpu(), conf.unsqueeze(1).cpu()


# ---------------------------------------------------------------------------------------------- one parametrised test per kind
@of_kind("aa")
def test_antialias_down_fp64_gate(hip, case):
    T, p = case.make(), case.p
    rows, got = run_aa(hip, case, T["x"].cuda())
    if p["s"] == 1:                                                     # the layout change alone: exact
        assert torch.equal(rows[:, :3].cpu(), mc.rows_of(T["x"]))
    want64 = gate(case, dict(out=got), T)
    err = G.rel_err(got, want64["out"])
    print(f"{case.name}: rel err {err:.3e}, format bound {G.aa_format_bound(p['s']):.3e}")
    assert err <= G.aa_format_bound(p["s"]), (case.name, err)          # sharper than the gate at s = 8: see aa_format_bound
    # the same frames as bytes: bit for bit the fp32 result of byte / 255
    _, u8 = run_aa(hip, case, T["u8"].cuda())
    assert torch.equal(u8, got), f"{case.name}: {int((u8 != got).sum())} values differ between bytes and byte / 255 planes"
    if p["clip"]:                                                       # a (3,T,H,W) clip permuted to frames: frame stride < channel stride
        clip = T["x"].permute(1, 0, 2, 3).contiguous().cuda().permute(1, 0, 2, 3)
        assert clip.stride(0) < clip.stride(1)
        assert torch.equal(run_aa(hip, case, clip)[1], got)


@of_kind("rm")
def test_region_moments_fp64_gate(hip, case):
    T, p = case.make(), case.p
    shift, covar, affine = hip.region_moments(T["rows"].cuda(), 2, p["h"], p["w"], p["R"], G.TEMPERATURE)
    want64 = gate(case, dict(shift=shift, covar=covar), T)
    assert torch.equal(covar[..., 0, 1], covar[..., 1, 0])
    G.check_affine(affine, want64["covar"], f"{case.name} affine")


def test_region_moments_isotropic_region(hip):
    rows, h, w, R, covar64 = G.rm_isotropic()
    shift, covar, affine = hip.region_moments(rows.cuda(), 1, h, w, R, G.TEMPERATURE)
    a = affine.double().cpu()
    assert bool(torch.isfinite(a).all()) and bool((torch.det(a) < 0).all())
    mc.assert_close(covar, covar64, "isotropic covar")
    mc.assert_close(a @ a.transpose(-1, -2), covar64, "isotropic A A^T = covar")


@of_kind("bg")
def test_bg_params_fp64_gate(hip, case):
    T, p = case.make(), case.p
    x = T["rows"].cuda()[:, :p["C"]]
    assert x.stride(0) == p["ld"]
    got = hip.bg_params(x, 2, T["fc_w"].cuda(), T["fc_b"].cuda())
    gate(case, dict(out=got), T)
    assert torch.equal(got[:, 2].cpu(), torch.tensor([0.0, 0.0, 1.0]).expand(2, 3))


@of_kind("mi")
def test_motion_inputs_fp64_gate(hip, case):
    T, p = case.make(), case.p
    rows = hip.motion_inputs(cu(T["drv"]), cu(T["src"]), T["bg"].cuda(), T["src_rows"].cuda(), T["T"], p["h"], p["w"], p["c_pad"])
    got = mi_maps(case, rows, T["T"])
    assert not bool(got["heat"][:, 0].any())                            # the background has no heatmap
    gate(case, got, T)


@of_kind("fc")
def test_flow_combine_fp64_gate(hip, case):
    T = case.make()
    rows, drv, src, bg = T["rows"].cuda(), cu(T["drv"]), cu(T["src"]), T["bg"].cuda()
    flow, occ = run_fc(hip, case, T, rows, drv, src, bg, False)
    flow_x0, occ_x0 = run_fc(hip, case, T, rows, drv, src, bg, True)
    assert torch.equal(flow_x0, flow)
    gate(case, dict(flow=flow, occ=occ, occ_x0=occ_x0), T)


# ---------------------------------------------------------------------------------------------- dawn_motion_inputs with ld_out > c_pad
@pytest.mark.parametrize("name", ["mi/exact_9x17_R10_cpad64", "mi/random_17x33_R10_cpad44"])
def test_motion_inputs_c_entry_leaves_the_columns_past_c_pad(hip, name):
    """The wrapper always allocates ld_out == c_pad; the C entry takes a wider row.  Every column past c_pad of a pre-filled buffer must
    come back untouched (the ragged last workgroup included), the others equal to the wrapper's result."""
    from dawn_pytorch_amd._lib import check
    case = case_named(name)
    T, p = case.make(), case.p
    n, h, w, c_pad = T["T"], p["h"], p["w"], p["c_pad"]
    assert (h * w) % 64
    drv, src, bg, src_rows = cu(T["drv"]), cu(T["src"]), T["bg"].cuda(), T["src_rows"].cuda()
    want = hip.motion_inputs(drv, src, bg, src_rows, n, h, w, c_pad)
    FILL, ld_out = 12345.675, c_pad + 8
    out = torch.full((n * h * w, ld_out), FILL, device="cuda")
    ptr = [t.data_ptr() for t in (*drv, *src, bg)]
    check(hip.L.dawn_motion_inputs(*ptr, p["R"], src_rows.data_ptr(), src_rows.stride(0), n, h, w, out.data_ptr(), ld_out, c_pad, hip._stream()),
          "dawn_motion_inputs")
    torch.cuda.synchronize()
    assert torch.equal(out[:, c_pad:], torch.full_like(out[:, c_pad:], FILL)), f"{name}: columns past c_pad were written"
    assert torch.equal(out[:, :c_pad], want)


# ---------------------------------------------------------------------------------------------- one ragged case per kernel between guard bands
def test_ragged_cases_between_guard_bands():
    """A write past a partial tile or a ragged tail trips a band; a read past src_rows, a row's R columns or C channels brings NaN into a
    result.  The results are the unguarded ones, gated again."""
    g = GuardedOps()
    # antialias_down: one partial tile, fp32 planes and bytes
    aa = case_named("aa/s4_37x50")
    Ta = aa.make()
    H, W = aa.p["H"], aa.p["W"]
    planes, _ = g.guarded_in(Ta["x"].reshape(2 * 3, H * W), name="planes")
    _, down = run_aa(g, aa, planes.view(2, 3, H, W))
    bytes_in, _ = g.guarded_in(Ta["u8"].reshape(2, -1), name="bytes")
    _, down_u8 = run_aa(g, aa, bytes_in.view(2, H, W, 3))
    # region_moments: 260 pixels = one stride of 256 and four
    rm = case_named("rm/13x20_R10")
    Tr = rm.make()
    rows_in, _ = g.guarded_in(Tr["rows"], name="regions")
    shift, covar, affine = g.region_moments(rows_in, 2, rm.p["h"], rm.p["w"], rm.p["R"], G.TEMPERATURE)
    # bg_params: C = 300 of ld = 304
    bg = case_named("bg/C300_npix9_ld304")
    Tb = bg.make()
    last_in, _ = g.guarded_in(Tb["rows"], name="bg_last")
    fcw_in, _ = g.guarded_in(Tb["fc_w"], name="fc_w")
    bgp = g.bg_params(last_in[:, :bg.p["C"]], 2, fcw_in, Tb["fc_b"].cuda())
    # motion_inputs and flow_combine: 153 pixels = 2 x 64 + 25, R = 15 (no zero quad; row[16] is read)
    mi, fc = case_named("mi/exact_9x17_R15_cpad64"), case_named("fc/exact_9x17_R15")
    Tm, Tf = mi.make(), fc.make()
    n, h, w, R = Tm["T"], mi.p["h"], mi.p["w"], mi.p["R"]
    drv_p = tuple(g.guarded_in(t.reshape(n * R, -1), name=f"drv{i}")[0].view(t.shape) for i, t in enumerate(Tm["drv"]))
    src_p = tuple(g.guarded_in(t.reshape(R, -1), name=f"src{i}")[0].view(t.shape) for i, t in enumerate(Tm["src"]))
    bg_in = g.guarded_in(Tm["bg"].reshape(n, 9), name="bg")[0].view(n, 3, 3)
    srows_in, _ = g.guarded_in(Tm["src_rows"], name="src_rows")
    rows = g.motion_inputs(drv_p, src_p, bg_in, srows_in, n, h, w, mi.p["c_pad"])
    mo_in, _ = g.guarded_in(Tf["rows"], name="mask_occ")
    grid = g.guarded_out(2 * n, h * w, name="grid").view(2, n, h, w)
    conf = g.guarded_out(n, h * w, name="conf").view(n, h, w)
    g.flow_combine(mo_in, drv_p, src_p, bg_in, n, h, w, grid, conf)
    torch.cuda.synchronize()
    g.verify()
    g.inputs_intact()
    names = {r.name for r in g.outs}
    assert {"antialias_down.out", "region_moments.shift", "region_moments.covar", "region_moments.affine", "bg_params.out",
            "motion_inputs.out", "grid", "conf"} <= names, names
    assert torch.equal(down, down_u8)
    gate(aa, dict(out=down), Ta)
    gate(rm, dict(shift=shift, covar=covar), Tr)
    gate(bg, dict(out=bgp), Tb)
    gate(mi, mi_maps(mi, rows, n), Tm)
    occ = conf.unsqueeze(1).cpu()
    gate(fc, dict(flow=grid.permute(1, 2, 3, 0).cpu(), occ=occ, occ_x0=2 * occ.double() - 1), Tf)


# ---------------------------------------------------------------------------------------------- non-square, end to end
@pytest.fixture(scope="module")
def encoder(hip):
    from dawn_pytorch_amd.motion_encoder import MotionEncoder
    sds = mc.state_dicts()
    return MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cuda", ops=hip)


def test_encode_clip_non_square_matches_the_reference_from_python_and_from_c(encoder):
    g = mc.golden("N")
    c = mc.E2E_CASES["N"]
    T, h, w = c["T"], c["H"] // mc.S, c["W"] // mc.S
    assert h != w and set(g) == {"optical_flow", "occlusion_map"}
    src_u8, drv_u8 = mc.frames_u8("N")
    src, drv = mc.to_float(src_u8).cuda(), mc.to_float(drv_u8).cuda()
    out = encoder.encode_clip(src, drv)
    assert out["real_vid_grid"].shape == (1, 2, T, h, w) and out["real_vid_conf"].shape == (1, 1, T, h, w)
    mc.assert_close(out["real_vid_grid"][0].permute(1, 2, 3, 0), g["optical_flow"], "N encode_clip optical_flow")
    mc.assert_close(out["real_vid_conf"][0, 0].unsqueeze(1), g["occlusion_map"], "N encode_clip occlusion_map")
    via = encoder.encode_clip(src, drv, via_c=True)
    assert torch.equal(via["real_vid_grid"], out["real_vid_grid"]) and torch.equal(via["real_vid_conf"], out["real_vid_conf"])
    u8 = encoder.encode_clip(src, torch.from_numpy(drv_u8).cuda(), via_c=True)                # bytes in
    assert torch.equal(u8["real_vid_grid"], out["real_vid_grid"]) and torch.equal(u8["real_vid_conf"], out["real_vid_conf"])
