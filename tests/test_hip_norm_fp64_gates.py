"""-m gpu: the streaming kernels of csrc/norm.hip (GroupNorm statistics on both finalisation paths, gn_apply_res, the LayerNorm row
statistics) and the boundary kernels of csrc/misc.hip (init_conv_x on the persistent MFMA kernel and the generic one, head_out) against a
float64 reference at fp32 accuracy (tests/norm_gate.py), on every branch of their launch code: the flush of GroupNorm's fp32 runs, a
channel quad that spans groups, column slices, blocks without rows, both loops of gn_reduce_block on both sides of their thresholds,
the second trip of every grid-stride loop, R = 4 rows per lane group and its tail, ragged quad counts, a second tile per workgroup,
frame sub-ranges, Co up to 256 and one head alone.

The gate (split_gate.fp32_gate): max|hip - fp64| / max|fp64| <= c x the same for the op in fp32 on the CPU + FLOOR, c = C_GATE = 2 unless
norm_gate.C_WIDE widens it with the MI355X measurement beside it.  tests/test_norm_gate_cpu.py shows that every case rejects the defects
of its branch.  Each gate appends its errors and its ratio to CPU fp32 to the op-error log."""
import pytest
import torch

import norm_gate as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def cu(t):
    return None if t is None else t.cuda()


def of_kind(*kinds):
    cs = [c for c in N.CASES if c.kind in kinds]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(rc, what):
    from dawn_pytorch_amd._lib import check
    check(rc, what)


@of_kind("gn_stats")
def test_gn_stats_fp64_gate(hip, case):
    """dawn_gn_partial on the case's grid, then both finalisations: dawn_gn_reduce_finalize through HipOps.gn_coeffs (with its own
    statistics pass where the case uses the grid gn_coeffs chooses) and dawn_gn_reduce + dawn_gn_finalize."""
    T, p = case.make(), case.p
    want64, base32 = case.want64(T), case.base32(T)
    wide = cu(T["wide"])
    x = case.x_of(dict(wide=wide))
    rows, C = x.shape
    assert x.stride(0) == p.get("ld", C)
    gamma, beta, fs, fsh = (cu(T[k]) for k in ("gamma", "beta", "fs", "fsh"))
    film = None if fs is None else (fs, fsh)
    nblk, s, L = case.nblk(), hip._stream(), hip.L
    part = torch.full((nblk, 16), float("nan"), device="cuda", dtype=torch.float64)         # a block without rows must still write its zeros
    ok(L.dawn_gn_partial(ptr(x), rows, C, x.stride(0), ptr(part), nblk, s), "dawn_gn_partial")
    total = p.get("total_rows", rows)
    a, b = hip.gn_coeffs(x, gamma, beta, film, total, N.EPS, part=part if p.get("nblk") else None)
    sums, a2, b2 = torch.empty(16, device="cuda", dtype=torch.float64), torch.empty_like(a), torch.empty_like(b)
    ok(L.dawn_gn_reduce(ptr(part), nblk, ptr(sums), s), "dawn_gn_reduce")
    ok(L.dawn_gn_finalize(ptr(sums), case.count(), ptr(gamma), ptr(beta), ptr(fs), ptr(fsh), C, N.EPS, ptr(a2), ptr(b2), s), "dawn_gn_finalize")
    torch.cuda.synchronize()
    assert torch.equal(wide.cpu(), T["wide"]), f"{case.name}: input modified"
    case.check("sums", sums, want64, base32)
    for tag, aa, bb in (("", a, b), ("two_step_", a2, b2)):
        case.check("a", aa, want64, base32, tag)
        case.check("b", bb, want64, base32, tag)


@of_kind("gn_reduce")
def test_gn_reduce_fp64_gate(hip, case):
    """Integer-valued partials: dawn_gn_reduce's sums bit for bit, dawn_gn_reduce_finalize's coefficients through the gate."""
    T, n, C = case.make(), case.p["nblk"], 64
    want64, base32 = case.want64(T), case.base32(T)
    part, gamma, beta, fs, fsh = (cu(T[k]) for k in ("part", "gamma", "beta", "fs", "fsh"))
    sums = torch.full((16,), float("nan"), device="cuda", dtype=torch.float64)
    a, b = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    s, L = hip._stream(), hip.L
    ok(L.dawn_gn_reduce(ptr(part), n, ptr(sums), s), "dawn_gn_reduce")
    ok(L.dawn_gn_reduce_finalize(ptr(part), n, case.count(), ptr(gamma), ptr(beta), ptr(fs), ptr(fsh), C, N.EPS, ptr(a), ptr(b), s),
       "dawn_gn_reduce_finalize")
    torch.cuda.synchronize()
    case.check("sums_exact", sums, want64, base32)
    case.check("a", a, want64, base32)
    case.check("b", b, want64, base32)


@of_kind("gn_apply")
def test_gn_apply_res_fp64_gate(hip, case):
    T, p = case.make(), case.p
    x, res = cu(T["x"]), cu(T["res"])
    got = hip.gn_apply_res(x, cu(T["a"]), cu(T["b"]), res, inplace=bool(p.get("inplace")))
    torch.cuda.synchronize()
    assert (got.data_ptr() == x.data_ptr()) == bool(p.get("inplace"))
    case.check("y", got, case.want64(T), case.base32(T))
    if not p.get("inplace"):
        assert torch.equal(x.cpu(), T["x"]), f"{case.name}: input modified"


@of_kind("ln")
def test_ln_rowstats_and_rows_fp64_gate(hip, case):
    T = case.make()
    want64, base32 = case.want64(T), case.base32(T)
    in0, in1 = case.ln_sources(dict(w0=cu(T["w0"]), w1=cu(T["w1"])))
    assert in0.stride(0) == case.p.get("ld0", case.p["C0"]) and (in1 is None or in1.stride(0) == case.p.get("ld1", case.p["C1"]))
    mean, rstd = hip.ln_rowstats(in0, in1, N.EPS)
    xn = hip.ln_rows(in0, in1, N.EPS)
    torch.cuda.synchronize()
    for key, got in (("mean", mean), ("rstd", rstd), ("xn", xn)):
        case.check(key, got, want64, base32)


@of_kind("first")
def test_init_conv_x_fp64_gate(hip, case):
    T, p = case.make(), case.p
    got = hip.init_conv_x(cu(T["x"]), cu(T["w3"]), cu(T["fea_pre"]), p["F"], p["h"], p["w"], p.get("Co", 64), frames=p.get("frames"))
    torch.cuda.synchronize()
    fa, fb = case.fsub()
    assert tuple(got.shape) == ((fb - fa) * p["h"] * p["w"], p.get("Co", 64))
    case.check("out", got, case.want64(T), case.base32(T))


@of_kind("head")
def test_head_out_fp64_gate(hip, case):
    """Both heads, and each alone into a pre-filled buffer whose other rows come back bit for bit."""
    T, which = case.make(), case.p["which"]
    out = None if which == "both" else cu(T["prefill"]).clone()
    got = hip.head_out(cu(T["hg"]), cu(T["ho"]), cu(T["wg"]), cu(T["bg"]), cu(T["wo"]), cu(T["bo"]), out=out)
    torch.cuda.synchronize()
    case.check("eps", got, case.want64(T), case.base32(T))
    if which == "g":
        assert torch.equal(got.cpu()[2:], T["prefill"][2:]), f"{case.name}: the absent head's row was written"
    if which == "o":
        assert torch.equal(got.cpu()[:2], T["prefill"][:2]), f"{case.name}: the absent head's rows were written"
