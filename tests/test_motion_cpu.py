"""No-GPU checks of the LFG motion encode: the float64 restatement of tests/motion_cases.py against every stage golden (the reference's
own stage outputs, from its own upstream values), the C entry points' refusals, the packer's channel padding, and MotionEncoder's
packing and orchestration under the CPU op set against the reference's end-to-end outputs."""
import ctypes as C

import pytest
import torch

import motion_cases as mc
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.motion_encoder import MotionEncoder, pad16, pad_conv_weight, unpad_conv_weight


@pytest.fixture(scope="module")
def sds():
    return mc.state_dicts()


@pytest.fixture(scope="module", params=list(mc.CASES))
def case(request):
    return request.param, mc.golden(request.param)


def test_input_formula_is_bytes_that_move():
    src, drv = mc.frames_u8("A")
    assert src.shape == (96, 96, 3) and drv.shape == (5, 96, 96, 3) and src.dtype == drv.dtype == "uint8"
    assert (src != drv[0]).any() and (drv[0] != drv[4]).any() and int(drv.max()) - int(drv.min()) > 200


def test_restatement_agrees_with_every_stage_golden(case):
    name, g = case
    c = mc.CASES[name]
    T, h, w = c["T"], c["H"] // mc.S, c["W"] // mc.S
    src_u8, drv_u8 = mc.frames_u8(name)
    # antialias_down
    mc.assert_close(mc.antialias_down(mc.to_float(src_u8).unsqueeze(0), mc.S)[0], g["down_src"], f"{name} down_src")
    if "down_drv" in g:
        mc.assert_close(mc.antialias_down(mc.to_float(drv_u8), mc.S), g["down_drv"], f"{name} down_drv")
    # region_moments
    pairs = [("drv", g["drv_regions"])] + ([("src", g["src_regions"])] if "src_regions" in g else [])
    for who, x in pairs:
        n = x.shape[0]
        shift, covar, affine = mc.region_moments(x.reshape(n, mc.R, h * w).transpose(1, 2), h, w)
        lead = (n,) if who == "drv" else ()
        mc.assert_close(shift.reshape(lead + (mc.R, 2)), g[f"{who}_shift"], f"{name} {who}_shift")
        mc.assert_close(covar.reshape(lead + (mc.R, 2, 2)), g[f"{who}_covar"], f"{name} {who}_covar")
        mc.check_affine(affine, covar, f"{name} {who}_affine")
        mc.check_affine(g[f"{who}_affine"], g[f"{who}_covar"], f"{name} {who}_affine of the reference")
        assert bool((torch.det(affine) < 0).all())                                          # the header's convention: det U = -1
    d_aff = mc.sqrt_factor(g["drv_covar"].double())
    s_aff = mc.sqrt_factor(g["src_covar"].double())
    mc.check_motion_matrices(s_aff.unsqueeze(0), d_aff, (g["src_covar"], g["src_affine"], g["src_u"]),
                             (g["drv_covar"], g["drv_affine"], g["drv_u"]), f"{name} M")
    drv, src = mc.region_params(g, "drv"), mc.region_params(g, "src")
    if name != "A":
        return
    # bg_params
    last = g["bg_last"]
    sd = mc.state_dicts()["bg_predictor"]
    mc.assert_close(mc.bg_params(last.flatten(2).transpose(1, 2), sd["fc.weight"], sd["fc.bias"]), g["bg_params"], "A bg_params")
    # motion_inputs, flow_combine
    fr = g["pf_in_frames"].tolist()
    mc.assert_close(mc.motion_inputs(drv, src, g["bg_params"], g["down_src"])[fr], g["pf_in"], "A pf_in")
    flow, occ = mc.flow_combine(g["mask_occ"], drv, src, g["bg_params"])
    mc.assert_close(flow, g["optical_flow"], "A optical_flow")
    mc.assert_close(occ, g["occlusion_map"], "A occlusion_map")


def test_abi_is_8_and_the_new_symbols_exist():
    L = _lib.lib()
    assert L.dawn_abi_version() == 8
    for n in ("dawn_antialias_down", "dawn_region_moments", "dawn_bg_params", "dawn_motion_inputs", "dawn_flow_combine"):
        assert hasattr(L, n) and n in _lib.SIGNATURES


P = 4096          # a non-NULL pointer that a refused call never dereferences


def _refused(fn, args, word):
    L = _lib.lib()
    assert getattr(L, fn)(*args) != 0, (fn, word)
    msg = L.dawn_last_error().decode()
    assert msg.startswith(fn + ":") and word in msg, (fn, word, msg)


def test_every_bad_argument_is_refused_by_name():
    """Refusals come before the first launch: no device is needed, and the dummy pointers are never read."""
    good = dict(
        dawn_antialias_down=[P, 0, 3 * 64, 64, 1, 8, 8, 4, P, 16, 16, None],
        dawn_region_moments=[P, 16, 1, 8, 8, 10, 0.1, P, P, P, None],
        dawn_bg_params=[P, 32, 1, 4, 32, P, P, P, None],
        dawn_motion_inputs=[P, P, P, P, P, P, P, 10, P, 16, 1, 8, 8, P, 48, 48, None],
        dawn_flow_combine=[P, 16, P, P, P, P, P, 10, 1, 8, 8, P, 64, P, 0, None])
    bad = dict(
        dawn_antialias_down=[(0, None, "in is NULL"), (8, None, "out is NULL"), (1, 2, "in_kind"), (4, 0, "T ="), (5, 0, "H ="), (7, 9, "s ="),
                             (2, 10, "frame_stride"), (3, 10, "chan_stride"), (10, 2, "c_pad"), (9, 8, "ld_out")],
        dawn_region_moments=[(0, None, "x is NULL"), (7, None, "shift is NULL"), (8, None, "covar is NULL"), (9, None, "affine is NULL"),
                             (5, 16, "R ="), (1, 9, "ld ="), (2, 0, "T ="), (3, 1, "h ="), (4, 1, "w ="), (6, 0.0, "temperature")],
        dawn_bg_params=[(0, None, "x is NULL"), (5, None, "fc_w is NULL"), (6, None, "fc_b is NULL"), (7, None, "out is NULL"), (2, 0, "T ="),
                        (3, 0, "npix"), (4, 0, "C ="), (1, 31, "ld =")],
        dawn_motion_inputs=[(0, None, "drv_shift is NULL"), (1, None, "drv_covar is NULL"), (2, None, "drv_affine is NULL"),
                            (3, None, "src_shift is NULL"), (4, None, "src_covar is NULL"), (5, None, "src_affine is NULL"),
                            (6, None, "bg_params is NULL"), (8, None, "src_rows is NULL"), (13, None, "out is NULL"), (7, 0, "R ="),
                            (10, 0, "T ="), (11, 1, "h ="), (12, 1, "w ="), (9, 2, "ld_src"), (15, 40, "c_pad"), (14, 44, "ld_out"),
                            (13, P + 4, "16-byte aligned")],
        dawn_flow_combine=[(0, None, "x is NULL"), (2, None, "drv_shift is NULL"), (3, None, "drv_affine is NULL"), (4, None, "src_shift is NULL"),
                           (5, None, "src_affine is NULL"), (6, None, "bg_params is NULL"), (11, None, "grid is NULL"), (13, None, "conf is NULL"),
                           (7, 16, "R ="), (8, 0, "T ="), (9, 1, "h ="), (1, 11, "ld ="), (12, 63, "grid_plane"), (14, 2, "conf_x0")])
    assert set(bad) == set(good)
    for fn, cases in bad.items():
        for pos, value, word in cases:
            args = list(good[fn])
            args[pos] = value
            _refused(fn, args, word)


def test_packer_round_trips_channel_padding():
    w = torch.arange(5 * 14 * 3 * 3, dtype=torch.float32).reshape(5, 14, 3, 3) + 1
    segs = [(8, 16), (3, 16), (3, 32)]
    wp = pad_conv_weight(w, segs, pad16(5))
    assert wp.shape == (16, 64, 3, 3)
    assert torch.equal(unpad_conv_weight(wp, segs, 5), w)
    assert float(wp.abs().sum()) == float(w.abs().sum())                                      # everything else is zero
    assert torch.equal(wp[:5, 16:19], w[:, 8:11]) and not bool(wp[5:].any()) and not bool(wp[:, 8:16].any())
    with pytest.raises(ValueError):
        pad_conv_weight(w, [(8, 16)], 16)


def test_unshipped_configurations_are_refused(sds):
    rp = dict(sds["region_predictor"])
    rp["jacobian.weight"] = torch.zeros(4, 11, 7, 7)
    with pytest.raises(ValueError, match="pca_based"):
        MotionEncoder(sds["generator"], rp, sds["bg_predictor"], "cpu", ops=mc.MotionRefOps())
    bg = dict(sds["bg_predictor"])
    bg["fc.weight"] = torch.zeros(8, 32)
    with pytest.raises(ValueError, match="affine"):
        MotionEncoder(sds["generator"], sds["region_predictor"], bg, "cpu", ops=mc.MotionRefOps())
    gen = {k: v for k, v in sds["generator"].items() if "occlusion" not in k}
    with pytest.raises(ValueError, match="occlusion"):
        MotionEncoder(gen, sds["region_predictor"], sds["bg_predictor"], "cpu", ops=mc.MotionRefOps())


def test_orchestration_matches_the_reference_end_to_end(sds):
    """MotionEncoder under the CPU op set (float32 convolutions, the restatement for the five kernels) against the reference's optical
    flow and occlusion map; the frames as bytes and as fp32 planes; the latent's third plane in the x0 convention."""
    g = mc.golden("A")
    T = mc.CASES["A"]["T"]
    src_u8, drv_u8 = mc.frames_u8("A")
    me = MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cpu", ops=mc.MotionRefOps())
    assert me.R == mc.R and me.s == mc.S
    src, drv = mc.to_float(src_u8), mc.to_float(drv_u8)
    out = me.encode_clip(src, drv)
    assert out["real_vid_grid"].shape == (1, 2, T, 24, 24) and out["real_vid_conf"].shape == (1, 1, T, 24, 24)
    mc.assert_close(out["real_vid_grid"][0].permute(1, 2, 3, 0), g["optical_flow"], "orchestration optical_flow")
    mc.assert_close(out["real_vid_conf"][0, 0].unsqueeze(1), g["occlusion_map"], "orchestration occlusion_map")
    u8 = me.encode_clip(torch.from_numpy(src_u8).unsqueeze(0), torch.from_numpy(drv_u8), chunk=2)
    mc.assert_close(u8["real_vid_grid"], out["real_vid_grid"], "bytes in, chunk 2")
    lat = me.latent(src, drv.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3))          # a (3,T,H,W) clip, permuted
    assert lat.shape == (3, T, 24, 24)
    mc.assert_close(lat[:2], out["real_vid_grid"][0], "latent grid")
    mc.assert_close(lat[2], 2 * out["real_vid_conf"][0, 0] - 1, "latent x0 plane")
