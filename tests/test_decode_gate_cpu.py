"""The fp32-accuracy gates of tests/decode_gate.py (the flow decoder's launches) can fail: every case, built with the same inputs as the GPU
test, ACCEPTS the op evaluated in fp32 on the CPU and REJECTS each defect decode_gate lists for it -- a lost or stale third weight plane, a
lost K chunk or tap, a tile's halo read as zero, a wrapped patch, a sampling position off by 1e-4 pixel, border clamp for zeros padding,
an unclamped resize index, a nearest occlusion, a missing ReLU, a misplaced up2 pixel -- emulated in float64 against the same reference
and checked with the case's own factor c: a factor widened until a defect passes fails here.  Also: the dyadic motion grids are exact in
fp32, the hooked float64 sampler is the oracle, and dawn_conv3x3_direct_form (host code) answers for every reduced conv case what it
answers for the production shape.  No GPU."""
import ctypes as C
import functools

import pytest
import torch

import decode_gate as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.policy import ConvPolicy as CP

IDS = [c.name for c in D.CASES]


@functools.lru_cache(maxsize=4)
def _refs(name):
    case = next(c for c in D.CASES if c.name == name)
    T = case.make()
    return case, T, case.want64(T), case.base32(T)


def of_kind(*kinds):
    cs = [c for c in D.CASES if c.kind in kinds]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def test_case_table_is_the_issue_s():
    """One case per launch / shape of the issue, and the defects each kind must carry."""
    kinds = {}
    for c in D.CASES:
        kinds.setdefault(c.kind, []).append(c)
    assert {k: len(v) for k, v in kinds.items()} == {"dconv": 12, "first": 3, "warp": 21, "final": 6, "ew": 5}
    assert len(set(IDS)) == len(IDS)
    for c in kinds["dconv"]:
        assert c.defect_names() == ("drop_third", "stale_third", "last_chunk_lost", "seam_halo_lost")
        assert c.p["H"] >= 3 * c.tile()[0] and c.p["C"] % 16 == 0          # three row tiles; dawn_conv_gemm's contract
    assert [(c.p["W"], c.p["C"], c.p["N"], 9 * c.p["C"]) for c in kinds["dconv"][:6]] == [
        (256, 64, 128, 576), (128, 128, 256, 1152), (64, 256, 256, 2304), (64, 256, 256, 2304), (128, 256, 128, 2304), (256, 128, 64, 1152)]
    assert [(c.p["W"], c.p["C"], c.p["N"]) for c in kinds["dconv"][6:]] == [
        (128, 64, 128), (64, 128, 256), (32, 256, 256), (32, 256, 256), (64, 256, 128), (128, 128, 64)]
    assert [bool(c.p["res"]) for c in kinds["dconv"]] == [False, False, False, True, False, False] * 2
    for c in kinds["first"]:
        assert c.defect_names() == ("trunc16", "last_tap_lost", "wrapped_patch")
    assert [(c.p["h"], c.p["w"]) for c in kinds["first"]] == [(8, 128), (8, 256), (8, 40)]
    for c in kinds["warp"]:          # a case lists the defects that can reach it, and no other
        resized, mode = c.p["S"] != c.p["s"], c.p["mode"]
        want = {"position_1e-4", "border_clamp"} | ({"resize_unclamped", "occ_nearest"} if resized else set())
        want |= ({"no_relu"} if mode in ("prev_ab", "prev_ab_up2") else set()) | ({"up2_neighbour"} if mode in ("prev_ab_up2", "prev_up2") else set())
        assert set(c.defect_names()) == want and c.p["C"] % 4 == 0, c.name
    assert {(c.p["S"], c.p["s"]) for c in kinds["warp"]} == {((16, 32), (16, 32)), ((32, 64), (16, 32)), ((64, 128), (16, 32)), ((16, 256), (4, 64))}
    for key in ("S", "mode"):        # every size and every mode meets every channel count
        for v in {c.p[key] for c in kinds["warp"]}:
            assert {c.p["C"] for c in kinds["warp"] if c.p[key] == v} == {4, 8, 64}, (key, v)
    assert {c.p["mode"] for c in kinds["warp"]} == set(D.WARP_MODES) and sum("view" in c.p for c in kinds["warp"]) == 1
    assert [(c.p["form"], c.p["H"], c.p["W"], c.p["C"]) for c in kinds["final"]] == [
        ("conv", 16, 32, 8), ("conv", 17, 33, 24), ("conv", 8, 8, 16), ("conv", 32, 64, 64), ("blend", 16, 32, 8), ("blend", 32, 64, 64)]
    for c in kinds["final"]:
        assert c.p["C"] % 8 == 0 and ("seam_halo_lost" in c.defect_names()) == ((c.p["H"], c.p["W"]) in ((17, 33), (32, 64)))
        assert c.defect_names()[:2] == ("last_chunk_lost", "tap_lost")
    assert all(c.defect_names() == () for c in kinds["ew"])
    assert all(c.c >= D.C_GATE for c in D.CASES)


@pytest.mark.parametrize("name", IDS)
def test_gate_accepts_cpu_fp32_and_rejects_defects(name):
    case, T, want64, base32 = _refs(name)
    assert want64.dtype == torch.float64 and base32.dtype == torch.float32 and want64.shape == base32.shape
    defects = case.defects(T, want64)
    assert tuple(defects) == case.defect_names()
    for i, out in enumerate(case.outputs()):
        w, b = (want64[i], base32[i]) if case.kind == "final" else (want64, base32)
        assert not D.gate_rejects(b, w, b, c=case.c)
        e32 = D.rel_err(b, w)
        # the baseline is an fp32 computation with a real fp32 error: never past fp32 accuracy, never exact
        assert 1e-9 < e32 < 2e-6, (out, e32)
        if i:
            continue                     # (the defects of a final case change out_vid)
        bound = case.c * e32 + D.FLOOR
        errs = {n: D.rel_err(t[0] if case.kind == "final" else t, w) for n, t in defects.items()}
        kept = {n: e for n, e in errs.items() if not e > bound}
        assert not kept, (case.name, f"bound {bound:.3e} (fp32 {e32:.3e}, c {case.c})", errs)


def direct_form(F, H, W, N, res=False, **kw):
    """dawn_conv3x3_direct_form of the descriptor FlowDecoder._conv3 builds (w_bf3 and bias, no Winograd images, the shipped policy).
    Host code: nothing is launched, the pointers are never dereferenced."""
    FAKE = 0x1000
    d = _lib.ConvDesc()
    d.in0, d.C0, d.ld0 = FAKE, kw["C"], kw["C"]
    d.F, d.Hi, d.Wi, d.Ho, d.Wo = F, H, W, H, W
    d.KH = d.KW = 3
    d.stride, d.pad, d.mode = 1, 1, 0
    d.w, d.bias, d.N, d.out, d.ld_out, d.w_bf3 = FAKE, FAKE, N, FAKE, N, FAKE
    if res:
        d.res, d.ld_res = FAKE, N
    return _lib.lib().dawn_conv3x3_direct_form(C.byref(d))


@of_kind("dconv")
def test_reduced_conv_case_takes_the_production_kernel(case):
    """Both shapes are listed in decode_gate.DCONV; the reduced one is minimal under its rule: with one frame less, or one row tile less,
    the launch lands on another instantiation or loses its third row tile."""
    prod, form, p = D.DCONV_PROD[case.name], D.DCONV_FORM[case.name], case.p
    assert direct_form(**prod) == form and direct_form(**p) == form, (case.name, direct_form(**prod), direct_form(**p))
    assert (p["W"], p["C"], p["N"], bool(p["res"])) == (prod["W"], prod["C"], prod["N"], prod["res"]) and p["F"] <= prod["F"] and p["H"] <= prod["H"]
    TR = case.tile()[0]
    if p["F"] > 1:
        assert direct_form(**dict(p, F=p["F"] - 1, H=prod["H"])) != form
    if p["H"] > 3 * TR:
        assert direct_form(**dict(p, H=p["H"] - TR)) != form


def test_direct_form_answers():
    """dawn_conv3x3_direct_form: 0 where the descriptor does not reach a direct split kernel, 1 the v1 halo kernel, 2 / 3 v2's tile widths."""
    base = dict(F=1, H=24, W=128, C=64, N=128)
    assert direct_form(**base) == D.V2_WN1
    assert direct_form(**dict(base, H=136, W=256)) == D.V2_WN2
    assert direct_form(**dict(base, F=3, H=5, W=64)) == 0                    # M % 64 != 0: neither v2 nor v1, the fp32 kernels
    assert _lib.lib().dawn_conv3x3_direct_form(None) == 0
    FAKE = 0x1000
    for change, want in (({}, D.V2_WN1), ({"w_bf3": 0}, 0), ({"policy": CP.DEFAULT & ~CP.SPLIT_V2}, D.HALO), ({"KH": 1, "KW": 1, "pad": 0}, 0),
                         ({"stride": 2}, 0), ({"w_wino": FAKE}, 0)):
        d = _lib.ConvDesc()
        d.in0, d.C0, d.ld0 = FAKE, 64, 64
        d.F, d.Hi, d.Wi, d.Ho, d.Wo = 4, 64, 64, 64, 64
        d.KH = d.KW = 3
        d.stride, d.pad, d.mode = 1, 1, 0
        d.w, d.N, d.out, d.ld_out, d.w_bf3 = FAKE, 64, FAKE, 64, FAKE
        for k, v in change.items():
            setattr(d, k, v)
        assert _lib.lib().dawn_conv3x3_direct_form(C.byref(d)) == want, change
        # the two queries never both claim a descriptor
        assert not (_lib.lib().dawn_conv3x3_form(C.byref(d)) and _lib.lib().dawn_conv3x3_direct_form(C.byref(d)))


@of_kind("warp")
def test_dyadic_motion_is_exact_and_hooked_sampler_is_the_oracle(case):
    """What the warp gate's sharpness rests on: the fp32 grid IS its float64 evaluation, CPU fp32 is within 3e-7 of float64 (2 x the largest
    measured, 1.44e-7: no position noise), less than half of the output rows are all zero, and warp64 without defects is RefOps.warp_blend."""
    case, T, want64, base32 = _refs(case.name)
    p = case.p
    Ttot, t0 = p.get("view", (3, 0))
    g64, _ = D.dyadic_grid64(Ttot, *p["s"], seed=p["S"][0] + p["C"] + len(p["mode"]), max_shift=p["shift"])
    assert torch.equal(T["grid"].double(), g64[:, t0:t0 + 3])
    if "view" in p:
        assert T["grid"].stride(0) == Ttot * p["s"][0] * p["s"][1] and not T["grid"].is_contiguous()
    assert D.rel_err(base32, want64) < 3e-7
    assert float((want64 == 0).all(dim=1).double().mean()) < 0.5
    got = case.hooked(T)
    assert got.dtype == torch.float64 and float((got - want64).abs().max() / want64.abs().max()) <= 1e-14


def test_dyadic_positions_are_exact_at_every_level():
    """The flows resized by 2 and by 4 and the sampling positions they give are the same numbers in fp32 and in float64."""
    import torch.nn.functional as F_
    grid, _ = D.dyadic_motion(3, 16, 32, seed=1, max_shift=3.0)
    for k in (1, 2, 4):
        Hs, Ws = 16 * k, 32 * k
        f32 = grid if k == 1 else F_.interpolate(grid.permute(1, 0, 2, 3), size=(Hs, Ws), mode="bilinear").permute(1, 0, 2, 3)
        f64 = grid.double() if k == 1 else F_.interpolate(grid.double().permute(1, 0, 2, 3), size=(Hs, Ws), mode="bilinear").permute(1, 0, 2, 3)
        assert f32.dtype == torch.float32 and torch.equal(f32.double(), f64)
        pos32 = ((f32[0] + 1) * Ws - 1) / 2
        assert torch.equal(pos32.double(), ((f64[0] + 1) * Ws - 1) / 2)


def test_identity_and_whole_pixel_motion_are_exact_in_the_oracle():
    """The expectations of the GPU file's exact-equality tests, on the fp32 oracle: bit for bit, no tolerance."""
    from oracle.ops_ref import RefOps
    for name, grid, conf, skip, want in D.exact_warp_cases(16, 32, 8):
        got = RefOps().warp_blend(skip, 16, 32, grid, conf)
        assert torch.equal(got, want), name


def test_trunc16_is_the_tf32_class_defect():
    x = D.rnd(4096, seed=5)
    t = D.trunc16(x)
    rel = ((x.double() - t) / x.double()).abs()
    assert bool((t.abs() <= x.double().abs()).all()) and float(rel.max()) < 2.0 ** -15 and float(rel.mean()) > 2.0 ** -19
