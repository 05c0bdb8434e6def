"""The fp32-accuracy gates of tests/motion_gate.py (the five kernels of the LFG motion encode) can fail: every case, built with the same
inputs as the GPU test, ACCEPTS the restatement evaluated in fp32 on the CPU and REJECTS each defect motion_gate lists for it -- an axis
swap, lost pixels, waves, channels, taps or halos, a wrong padding, divisor or kept pixel, a one-pass float32 covariance, a position off by
1e-4 pixel, a missing sign fix or division by Z ... -- emulated in float64 against the same reference and checked with the case's own
factor c: a factor widened until a defect passes fails here.  Each defect's error over its bound is printed.  Also the conditions on the
inputs that the gates' sharpness rests on: the eigen-gap floor of every region, CPU fp32 below 5e-7 on the exact-position family, whose
positions are the same numbers in fp32 and float64, samples outside the source, Z != 1, M[0][0] == 0 exactly; and the hooked float64
restatements are motion_cases'.  No GPU."""
import functools

import pytest
import torch

import motion_cases as mc
import motion_gate as G

IDS = [c.name for c in G.CASES]


@functools.lru_cache(maxsize=None)
def _refs(name):
    case = next(c for c in G.CASES if c.name == name)
    T = case.make()
    return case, T, case.want64(T), case.base32(T)


def of_kind(*kinds, **where):
    cs = [c for c in G.CASES if c.kind in kinds and all(c.p[k] == v for k, v in where.items())]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def test_case_table_is_the_issue_s():
    kinds = {}
    for c in G.CASES:
        kinds.setdefault(c.kind, []).append(c)
    assert {k: len(v) for k, v in kinds.items()} == {"aa": 6, "rm": 4, "bg": 4, "mi": 15, "fc": 15} and len(set(IDS)) == len(IDS)
    assert [(c.p["s"], c.p["H"], c.p["W"], c.out_hw()) for c in kinds["aa"]] == [
        (4, 37, 50, (10, 13)), (4, 70, 132, (18, 33)), (8, 136, 72, (17, 9)), (2, 33, 35, (17, 18)), (3, 50, 49, (17, 17)), (1, 7, 5, (7, 5))]
    assert sum(bool(c.p["clip"]) for c in kinds["aa"]) == 1
    for c in kinds["aa"]:
        assert ("halo_lost" in c.defect_names()) == (c.out_hw()[0] > 16) and "bytes_256" in c.defect_names()
        assert c.p["s"] == 1 or set(c.defect_names()) >= {"replicate_pad", "last_vtap_lost", "kept_plus_1"}
    assert [(c.p["h"], c.p["w"], c.p["R"]) for c in kinds["rm"]] == [(9, 17, 1), (17, 9, 15), (24, 40, 10), (13, 20, 10)]
    assert [c.defect_names() for c in kinds["rm"]] == [("axis_swap", "wave_lost", "f32_one_pass")] * 2 + [
        ("axis_swap", "tail_lost", "wave_lost", "f32_one_pass")] * 2
    assert [(c.p["C"], c.p["npix"], c.p["ld"]) for c in kinds["bg"]] == [(32, 144, 32), (300, 9, 304), (1024, 4, 1024), (1024, 1, 1040)]
    assert [c.defect_names() for c in kinds["bg"]] == [("mean_npix_1", "f32_sums"), ("channels_256_lost", "waves_1_3_lost", "mean_npix_1"),
                                                       ("channels_256_lost", "waves_1_3_lost", "mean_npix_1"), ("channels_256_lost", "waves_1_3_lost")]
    for kind, all_defects in (("mi", G.DEFECTS_MI), ("fc", G.DEFECTS_FC)):
        cs = kinds[kind]
        assert {(c.p["family"], c.p["h"], c.p["w"]) for c in cs} == {("exact", 9, 17), ("exact", 17, 33), ("random", 9, 17), ("random", 17, 33),
                                                                     ("random", 24, 40)}
        for key in ("family", "h"):
            for v in {c.p[key] for c in cs}:
                assert {c.p["R"] for c in cs if c.p[key] == v} == {1, 10, 15}
        for c in cs:          # a case lists the defects that can reach it, and no other: every grid is non-square, 24 x 40 has no ragged tail
            assert set(all_defects) - set(c.defect_names()) == ({"tail_zero"} if kind == "mi" and (c.p["h"], c.p["w"]) == (24, 40) else set()), c.name
    for R in (1, 10):         # every R meets c_pad = 4 (R + 1) and c_pad = 64 (at R = 15 they are the same)
        assert {c.p["c_pad"] for c in kinds["mi"] if c.p["R"] == R} == {4 * (R + 1), 64}
    assert all(c.p["c_pad"] == 64 for c in kinds["mi"] if c.p["R"] == 15)
    assert all(c.c(o) >= G.C_GATE for c in G.CASES for o in c.gated())


@pytest.mark.parametrize("name", IDS)
def test_gate_accepts_cpu_fp32_and_rejects_defects(name):
    case, T, want64, base32 = _refs(name)
    exact_op = case.kind == "aa" and case.p["s"] == 1                       # a layout change: fp32 is exact
    bound = {}
    for o in case.gated():
        w, b = want64[o], base32[o]
        assert w.dtype == torch.float64 and b.dtype == torch.float32 and w.shape == b.shape, o
        assert not G.gate_rejects(b, w, b, c=case.c(o))
        e32 = G.rel_err(b, w)
        # the baseline is an fp32 computation with a real fp32 error: never past fp32 accuracy, never exact
        assert (e32 == 0.0) if exact_op else (1e-9 < e32 < 1e-5), (o, e32)
        bound[o] = case.c(o) * e32 + G.FLOOR
        print(f"{name}/{o}: CPU fp32 rel err {e32:.3e}, bound {bound[o]:.3e} (c {case.c(o)})")
    defects = case.defects(T, want64)
    assert tuple(defects) == case.defect_names()
    kept = []
    for n, outs in defects.items():
        over = {o: G.rel_err(outs[o], want64[o]) / bound[o] for o in case.gated()}
        worst = max(over, key=lambda o: over[o] if over[o] == over[o] else float("inf"))
        print(f"{name}: defect {n}: err / bound {over[worst]:.3g} on {worst}")
        if not any(G.gate_rejects(outs[o], want64[o], base32[o], c=case.c(o)) or bool(torch.isnan(outs[o]).any()) for o in case.gated()):
            kept.append((n, over))
    assert not kept, (name, kept)


def test_format_bound_of_antialias_down_rejects_a_running_sum_divisor():
    """The divisor S = sum_ij fp32(g[i] g[j]) taken as a running float32 sum scales every output by S64 / S: 2.8e-6 at s = 8, which the
    fp32 gate at c = 2 passes (CPU fp32's own 841-tap convolution is at 1.4e-6) and motion_gate.aa_format_bound does not."""
    case, T, want64, base32 = _refs("aa/s8_136x72")
    run, exact = G.aa_running_sum_divisor(8)
    bad = want64["out"] * (exact / run)
    err = G.rel_err(bad, want64["out"])
    print(f"s = 8: running-sum divisor off by {(run - exact) / exact:.3e}; rel err {err:.3e}, format bound {G.aa_format_bound(8):.3e}, "
          f"fp32 gate bound {2 * G.rel_err(base32['out'], want64['out']) + G.FLOOR:.3e}")
    assert 2.5e-6 < err < 3.2e-6 and err > 2 * G.aa_format_bound(8)
    for c in G.CASES:                                                        # and the bound leaves fp32 arithmetic its room: > 5 ulps
        if c.kind == "aa":
            assert 5 * 2.0 ** -24 < G.aa_format_bound(c.p["s"]) < 1.2e-6


# ---------------------------------------------------------------------------------------------- conditions on the inputs
@of_kind("rm")
def test_every_region_keeps_its_eigen_gap_and_cpu_fp32_meets_the_affine_bound(case):
    case, T, want64, base32 = _refs(case.name)
    gap = mc.eigen_gap(want64["covar"])
    print(f"{case.name}: relative eigen-gap {float(gap.min()):.3g} .. {float(gap.max()):.3g}")
    assert float(gap.min()) >= G.RM_GAP_FLOOR                               # no region is ever skipped
    assert bool(torch.isnan(T["rows"][:, case.p["R"]:]).all()) and torch.equal(T["rows"][:, :case.p["R"]].reshape(T["x"].shape), T["x"])
    G.check_affine(base32["affine"], want64["covar"], f"{case.name} CPU fp32 affine")
    assert torch.equal(want64["affine"], mc.sqrt_factor(want64["covar"]))


def test_isotropic_region_is_isotropic():
    rows, h, w, R, covar64 = G.rm_isotropic()
    assert float(mc.eigen_gap(covar64).max()) < 1e-6 and float(covar64[..., 0, 1].abs().max()) < 1e-12
    a = mc.sqrt_factor(covar64)
    mc.assert_close(a @ a.transpose(-1, -2), covar64, "isotropic A A^T")
    assert bool((torch.det(a) < 0).all())


@of_kind("bg")
def test_bg_activations_are_relu_like(case):
    _, T, _, _ = _refs(case.name)
    x = T["x"]
    floor = x.amin(dim=(0, 1)) if case.p["npix"] > 4 else None
    assert float(x.min()) >= 0 and float(x.mean(dim=(0, 1)).std()) > 0.05                 # non-negative, a per-channel offset
    if floor is not None:                                                                # most pixels sit on their channel's floor
        assert 0.5 < float((x == floor).float().mean()) < 0.95
    assert T["rows"].shape[1] == case.p["ld"] and (case.p["ld"] == case.p["C"] or bool(torch.isnan(T["rows"][:, case.p["C"]:]).all()))


@of_kind("mi", "fc")
def test_motion_parameters_reach_every_branch(case):
    case, T, want64, base32 = _refs(case.name)
    p, (h, w, R) = case.p, (case.p["h"], case.p["w"], case.p["R"])
    drv, src, bg, slots, n = T["drv"], T["src"], T["bg"], T["slots"], T["T"]
    assert n == (2 if R >= 3 else 4) and all(t >= 1 for t, _ in slots.values()) and max(t for t, _ in slots.values()) == n - 1
    M64 = src[2].double().unsqueeze(0) @ torch.inverse(drv[2].double())     # before the sign fix
    M32 = src[2].unsqueeze(0) @ torch.inverse(drv[2])
    t, r = slots["neg"]
    assert float(M64[t, r, 0, 0]) < -0.1 and float(M32[t, r, 0, 0]) < -0.1
    t, r = slots["zero"]
    assert float(M64[t, r, 0, 0]) == 0.0 and float(M32[t, r, 0, 0]) == 0.0 and float(M64[t, r].abs().max()) > 0.1
    assert not bool(mc.motion_matrix(src[2][r], drv[2][t, r]).any())        # zeroed, as torch.sign does
    m = G.motions64(drv, src, bg, h, w)
    t, r = slots["outside"]
    ix, iy = ((m[t, r + 1, ..., 0] + 1) * w - 1) / 2, ((m[t, r + 1, ..., 1] + 1) * h - 1) / 2
    assert bool(((ix <= -1) | (ix >= w) | (iy <= -1) | (iy >= h)).all())    # wholly outside
    share = G.outside_share(drv, src, bg, h, w)
    print(f"{case.name}: {share:.1%} of the samples fall outside the source")
    assert 0.05 < share < 0.7
    a, b = float(bg[n - 1, 2, 0]), float(bg[n - 1, 2, 1])
    assert 0 < abs(a) <= 0.1 and 0 < abs(b) <= 0.1 and float(bg[n - 1, 2, 2]) == 1.0
    gh = torch.cat((mc.coordinate_grid(h, w), torch.ones(h, w, 1, dtype=torch.float64)), 2)
    Z = gh @ bg[n - 1, 2].double()
    assert 0.8 <= float(Z.min()) < float(Z.max()) <= 1.2 and float((Z != 1).double().mean()) > 0.9
    assert bool((torch.det(drv[1].double()) > 0).all()) and bool((torch.det(src[1].double()) > 0).all())
    if p["family"] != "exact":
        return
    # the exact family: every region's sparse motion and sampling position is the same number in fp32 and in float64
    g32 = mc.coordinate_grid(h, w, torch.float32)
    gx = 2 * torch.arange(w, dtype=torch.float64) / (w - 1) - 1
    assert torch.equal(g32[0, :, 0].double(), gx)
    m32 = mc.sparse_motions(drv, src, bg, h, w, dtype=torch.float32)
    assert m32.dtype == torch.float32 and torch.equal(m32.double(), m)      # the background's too: its quotient is exact (motion_params)
    assert len(m[n - 1, 0].reshape(-1, 2).unique(dim=0)) == 1 and len(m[0, 0].reshape(-1, 2).unique(dim=0)) == h * w
    pos32 = ((m32[..., 0] + 1) * w - 1) / 2
    assert torch.equal(pos32.double(), ((m[..., 0] + 1) * w - 1) / 2)
    for o in (("warped",) if case.kind == "mi" else ("flow",)):
        e32 = G.rel_err(base32[o], want64[o])
        print(f"{case.name}/{o}: CPU fp32 on exact positions {e32:.3e}")
        assert e32 < G.EXACT_BASE32_MAX


@of_kind("mi")
def test_hooked_motion_inputs_is_the_restatement(case):
    case, T, want64, _ = _refs(case.name)
    got = G.split_mi(G.mi64(T["drv"], T["src"], T["bg"], T["src_down"]))
    for o in ("heat", "warped"):
        assert got[o].dtype == torch.float64 and float((got[o] - want64[o]).abs().max()) <= 1e-13, o
    assert bool(torch.isnan(T["src_rows"][:, 3:]).all()) and T["src_rows"].shape[1] == 16


@of_kind("fc")
def test_hooked_flow_combine_is_the_restatement(case):
    case, T, want64, _ = _refs(case.name)
    flow, occ = G.fc64(T["x"], T["drv"], T["src"], T["bg"])
    assert float((flow - want64["flow"]).abs().max()) <= 1e-13 and torch.equal(occ, want64["occ"])
    R = case.p["R"]
    assert T["rows"].shape[1] >= R + 2 and bool(torch.isnan(T["rows"][:, R + 2:]).all())


def test_position_error_stands_clear_on_the_exact_family_only():
    """What the exact family buys: a position off by 1e-4 pixel is ~1e-4 of the output either way, CPU fp32 is below 5e-7 on exact
    positions and 1e-6 .. 1e-5 on random ones."""
    for fam, lo, hi in (("exact", 0.0, G.EXACT_BASE32_MAX), ("random", 5e-7, 2e-5)):
        case, T, want64, base32 = _refs(f"mi/{fam}_17x33_R15_cpad64")
        e32 = G.rel_err(base32["warped"], want64["warped"])
        off = G.rel_err(G.split_mi(G.mi64(T["drv"], T["src"], T["bg"], T["src_down"], defect="position_1e-4"))["warped"], want64["warped"])
        print(f"{case.name}: CPU fp32 {e32:.3e}, position off by 1e-4 pixel {off:.3e}")
        assert lo < e32 < hi and 3e-5 < off < 1e-3


def test_restatement_in_float64_is_unchanged_by_the_dtype_argument():
    """The default of every dtype argument is float64, and float32 gives float32."""
    x = G.rnd(1, 3, 9, 10, seed=1)
    assert mc.antialias_down(x, 4).dtype == torch.float64 and mc.antialias_down(x, 4, dtype=torch.float32).dtype == torch.float32
    assert mc.coordinate_grid(3, 5).dtype == torch.float64
    assert torch.equal(mc.coordinate_grid(3, 5, torch.float32).double(), mc.coordinate_grid(3, 5))


# ---------------------------------------------------------------------------------------------- non-square, end to end
def test_orchestration_matches_the_reference_on_a_non_square_clip():
    """MotionEncoder under the CPU op set against the reference's own run on 96 x 128 frames (h = 24, w = 32): a swap of the two sides in
    the packing, the orchestration or the restatement cannot pass here."""
    from dawn_pytorch_amd.motion_encoder import MotionEncoder
    g = mc.golden("N")
    c = mc.E2E_CASES["N"]
    T, h, w = c["T"], c["H"] // mc.S, c["W"] // mc.S
    assert (h, w) == (24, 32) and set(g) == {"optical_flow", "occlusion_map"} and "N" not in mc.CASES
    assert tuple(g["optical_flow"].shape) == (T, h, w, 2) and tuple(g["occlusion_map"].shape) == (T, 1, h, w)
    src_u8, drv_u8 = mc.frames_u8("N")
    assert src_u8.shape == (96, 128, 3) and drv_u8.shape == (T, 96, 128, 3)
    sds = mc.state_dicts()
    me = MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cpu", ops=mc.MotionRefOps())
    out = me.encode_clip(mc.to_float(src_u8), mc.to_float(drv_u8))
    assert out["real_vid_grid"].shape == (1, 2, T, h, w) and out["real_vid_conf"].shape == (1, 1, T, h, w)
    mc.assert_close(out["real_vid_grid"][0].permute(1, 2, 3, 0), g["optical_flow"], "N orchestration optical_flow")
    mc.assert_close(out["real_vid_conf"][0, 0].unsqueeze(1), g["occlusion_map"], "N orchestration occlusion_map")
