"""The fp32-accuracy gates of tests/norm_gate.py (GroupNorm, LayerNorm, init_conv_x, head_out on every launch branch) can fail: every case,
built with the same inputs as the GPU test, ACCEPTS the op evaluated in fp32 on the CPU and REJECTS each defect norm_gate lists for it,
on every output the defect reaches, emulated in float64 against the same reference and checked with the case's own factor c: a factor
widened until a defect passes fails here.  Every emulator without a defect is the plain reference.  No GPU."""
import functools

import pytest
import torch

import norm_gate as N
from oracle.ops_ref import RefOps

IDS = [c.name for c in N.CASES]


@functools.lru_cache(maxsize=2)
def _refs(name):
    case = next(c for c in N.CASES if c.name == name)
    T = case.make()
    return case, T, case.want64(T), case.base32(T)


def of_kind(*kinds):
    cs = [c for c in N.CASES if c.kind in kinds]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def test_case_table_reaches_every_branch():
    """The cases sit on both sides of each threshold of the launch code, and each defect is attached exactly where it can reach."""
    kinds = {}
    for c in N.CASES:
        kinds.setdefault(c.kind, []).append(c)
    assert {k: len(v) for k, v in kinds.items()} == {"gn_stats": 15, "gn_reduce": 14, "gn_apply": 6, "ln": 15, "first": 10, "head": 6}
    assert len(set(IDS)) == len(IDS)
    assert all(c.c >= N.C_GATE for c in N.CASES)
    # ---- gn_stats
    gs = kinds["gn_stats"]
    assert {c.p["C"] for c in gs} == {8, 16, 32, 64, 512, 1024}
    assert {c.p["n"] for c in gs if c.p.get("n")} == {63, 64, 65, 128, 130} and all(c.nblk() in (1, 2) for c in gs if c.p.get("n"))
    for c in gs:
        names, p = c.defect_names(), c.p
        assert ("remainder_lost" in names) == (p.get("n") not in (64, 128)) and (not p.get("n") or c.thread_rows() == {p["n"]})
        assert ("quad_to_first_group" in names) == (p["C"] in (8, 16)) and ("ld_as_C" in names) == ("ld" in p)
        assert ("film_shift_first" in names) == bool(p.get("film")) and ("count_from_rows" in names) == ("total_rows" in p)
        assert names, c.name
    assert sum("ld" in c.p for c in gs) == 1 and sum("total_rows" in c.p for c in gs) == 1
    assert any(c.p.get("film") for c in gs) and any(not c.p.get("film") for c in gs)
    small = next(c for c in gs if c.name.endswith("C16_r200_nblk8"))
    assert small.p["rows"] < (small.nblk() - 4) * 64                               # four blocks of 64 rows per iteration see no row at all
    # ---- gn_reduce
    assert tuple(c.p["nblk"] for c in kinds["gn_reduce"]) == (1, 15, 16, 17, 240, 241, 256, 257, 511, 960, 961, 1024, 1025, 3200)
    for c in kinds["gn_reduce"]:
        n = c.p["nblk"]
        assert bool(N.in_unrolled(n, 256).any()) == (n > 240) and bool(N.in_unrolled(n, 1024).any()) == (n > 960)
        assert ("unrolled_dropped" in c.defect_names()) == (n > 240) and ("tail_dropped" in c.defect_names()) == (n != 1024)
    # ---- gn_apply
    quads = sorted(c.p["rows"] * (c.p["C"] // 4) for c in kinds["gn_apply"])
    assert N.GN_APPLY_QUADS - 64 in quads and N.GN_APPLY_QUADS in quads and N.GN_APPLY_QUADS + 64 in quads
    for c in kinds["gn_apply"]:
        assert (c.defect_names() == ("second_trip_lost",)) == (c.p["rows"] * (c.p["C"] // 4) > N.GN_APPLY_QUADS)
    assert {(bool(c.p.get("res")), bool(c.p.get("inplace"))) for c in kinds["gn_apply"] if c.defect_names()} == {(True, False), (False, True), (True, True)}
    assert any(c.p["C"] == 8 and c.defect_names() for c in kinds["gn_apply"]) and any(c.p["C"] == 8 and not c.defect_names() for c in kinds["gn_apply"])
    # ---- ln
    ln = kinds["ln"]
    assert sorted(c.p["rows"] for c in ln if c.p["C0"] == 16) == [65535, 65536, 65537, 65539]
    assert {(c.p["C0"], c.p.get("C1", 0)) for c in ln if c.r4()} == {(16, 0), (96, 0), (48, 80), (64, 64), (256, 0)}
    assert {(c.p["C0"], c.p.get("C1", 0)) for c in ln if not c.r4()} == {(16, 0), (8, 8), (24, 0), (28, 0), (40, 0), (1020, 0), (512, 512), (48, 80)}
    assert {c.lanes() for c in ln} == {4, 8, 16, 32, 64}
    assert {c.p["rows"] % 4 for c in ln if c.r4()} == {0, 1, 2, 3}
    for c in ln:
        names, C = c.defect_names(), c.p["C0"] + c.p.get("C1", 0)
        assert "onepass32" in names and ("second_from_first" in names) == bool(c.p.get("C1")) and ("pad_quads" in names) == (C != 1024)
        assert ("r4_rows_as_r1" in names) == (c.p["rows"] >= 65536) and ("r4_tail_zero" in names) == (c.p["rows"] in (65537, 65538, 65539))
        assert c.r4() or c.p["rows"] % (256 // c.lanes())                         # a partial last workgroup
    # ---- first
    fi = {c.name.split("/")[1]: c for c in kinds["first"]}
    assert [n for n, c in fi.items() if c.mfma()] == ["mfma_768x8x32", "mfma_770x8x32", "mfma_w8_2x64x8", "mfma_one_tile_3x4x64", "mfma_frames2-5of7_16x16"]
    assert fi["mfma_770x8x32"].tiles() == (770, 1) and all(c.tiles()[0] <= N.FIRST_SLOTS for n, c in fi.items() if c.mfma() and n != "mfma_770x8x32")
    assert fi["mfma_768x8x32"].tiles() == (N.FIRST_SLOTS, 1) and fi["generic_Co16_4x256x256"].threads() == N.FIRST_GENERIC_THREADS
    assert fi["mfma_w8_2x64x8"].tiles() == (4, 2) and fi["mfma_one_tile_3x4x64"].tiles() == (3, 1)
    assert fi["generic_stride_7x236x40"].threads() > N.FIRST_GENERIC_THREADS and 256 % 40
    assert all(c.threads() <= N.FIRST_GENERIC_THREADS for n, c in fi.items() if not c.mfma() and n != "generic_stride_7x236x40")
    assert {c.p.get("Co", 64) for c in fi.values() if not c.mfma()} == {16, 64, 96}
    for c in fi.values():
        names = c.defect_names()
        assert names[:3] == ("trunc16", "last_tap_lost", "wrapped_patch") and ("plane_stride" in names) == ("frames" in c.p)
        assert ("stale_patch" in names) == (c is fi["mfma_770x8x32"])
    assert {c.mfma() for c in fi.values() if "frames" in c.p} == {True, False}
    # ---- head
    assert {(c.p["Co"], c.p["which"]) for c in kinds["head"]} == {(Co, wh) for Co in (128, 256) for wh in ("both", "g", "o")}
    assert all(c.p["rows"] % 16 for c in kinds["head"])
    for c in kinds["head"]:
        assert c.defect_names() == ("channels_from_64_lost",) + (("absent_head_written",) if c.p["which"] != "both" else ())


@pytest.mark.parametrize("name", IDS)
def test_gate_accepts_cpu_fp32_and_rejects_defects(name):
    case, T, want64, base32 = _refs(name)
    gated = [k for k in want64 if case.mode(k) == "gate"]
    assert sorted(base32) == sorted(gated)
    for k in gated:
        assert want64[k].dtype == torch.float64 and base32[k].dtype == torch.float32 and want64[k].shape == base32[k].shape
        assert not case.rejects(k, base32[k], want64, base32)
        e32 = N.rel_err(base32[k], want64[k])
        # the baseline is an fp32 computation: a real error, never past fp32 accuracy (the largest, 1.5e-6: LayerNorm rows of DC offset
        # 12 and amplitude 0.25, where the mean's rounding of 1e-6 is multiplied by rstd = 4)
        assert 1e-9 < e32 < 5e-6, (case.name, k, e32)
    defects = case.defects(T, want64)
    assert tuple(defects) == case.defect_names()
    for dname, outs in defects.items():
        assert outs and set(outs) <= set(want64), (case.name, dname)
        kept = {k: N.rel_err(t, want64[k]) for k, t in outs.items() if not case.rejects(k, t, want64, base32)}
        assert not kept, (case.name, dname, f"c {case.c}", kept, {k: N.rel_err(base32[k], want64[k]) for k in gated})


@of_kind("gn_stats")
def test_gn_reference_arithmetic_stays_inside_the_gate(case):
    """Float64 sums followed by gn_coeff's fp32 finalisation -- a faultless kernel -- pass the gate on this data, and so does the
    kernel's own summation (fp32 runs of 64 rows per thread, emulated with its thread-to-row map); the 16 sums of that emulation stay
    within the floor of the float64 sums."""
    case, T, want64, base32 = _refs(case.name)
    for k, t in case.reference_arithmetic(T).items():
        assert t.dtype == torch.float32 and not case.rejects(k, t, want64, base32), (case.name, k, N.rel_err(t, want64[k]))
    sums = N.gn_partial_emul(case.x_of(T), case.nblk(), dtype=torch.float32)
    assert not case.rejects("sums", sums, want64, base32), N.rel_err(sums, want64["sums"])
    a, b = N.gn_coeff(sums, case.count(), T["gamma"], T["beta"], T["fs"], T["fsh"], fp32_final=True)
    assert not case.rejects("a", a, want64, base32) and not case.rejects("b", b, want64, base32)


@of_kind("gn_stats")
def test_gn_emulator_is_the_plain_reference(case):
    """gn_partial_emul without a defect = the plain float64 group sums; gn_coeff in float64 on them = RefOps.gn_coeffs in float64."""
    case, T, want64, _ = _refs(case.name)
    sums = N.gn_partial_emul(case.x_of(T), case.nblk())
    assert sums.dtype == torch.float64 and N.rel_err(sums, want64["sums"]) <= 1e-14
    x = case.x_of(T).double()
    film = None if T["fs"] is None else (T["fs"].double(), T["fsh"].double())
    a, b = RefOps().gn_coeffs(x, T["gamma"].double(), T["beta"].double(), film, case.p.get("total_rows", case.p["rows"]), eps=N.EPS)
    assert N.rel_err(a, want64["a"]) <= 1e-9 and N.rel_err(b, want64["b"]) <= 1e-9          # (eps: 1e-5 here, float(1e-5f) in gn_coeff)


@of_kind("gn_reduce")
def test_reduce_split_is_a_partition(case):
    """in_unrolled splits the partial rows as gn_reduce_block's two loops do (restated as the loops themselves), and both parts together
    are the exact sums."""
    n, part = case.p["nblk"], case.make()["part"]
    for NT in (256, 1024):
        NP, m = NT // 16, N.in_unrolled(n, NT)
        want = torch.zeros(n, dtype=torch.bool)
        for r in range(min(NP, n)):
            b = r
            while b + 15 * NP < n:
                want[b:b + 16 * NP:NP] = True
                b += 16 * NP
        assert torch.equal(m, want), (n, NT)
        assert torch.equal(part[m].sum(0) + part[~m].sum(0), part.sum(0)) and float(part.abs().sum()) < 2.0 ** 53
    assert torch.equal(part, part.round())


@of_kind("ln")
def test_ln_hooked_reference_is_the_oracle(case):
    case, T, want64, _ = _refs(case.name)
    in0, in1 = case.ln_sources(T)
    mean, rstd = RefOps().ln_rowstats(in0.double(), None if in1 is None else in1.double(), N.EPS)
    xn = RefOps().ln_rows(in0.double(), None if in1 is None else in1.double(), N.EPS)
    for k, t in (("mean", mean), ("rstd", rstd), ("xn", xn)):
        assert N.rel_err(t, want64[k]) <= 1e-13, k
    assert not in0.is_contiguous() or "ld0" not in case.p


def test_first_plane_stride_emulation_is_exact_at_the_true_stride():
    """The flat-memory read of the `plane_stride` defect, given the true stride F h w, is the frame sub-range itself."""
    case = next(c for c in N.CASES if c.name == "first/mfma_frames2-5of7_16x16")
    x = case.make()["x"]
    F, h, w = case.p["F"], case.p["h"], case.p["w"]
    fa, fb = case.fsub()
    flat = x.reshape(-1)[fa * h * w:]
    assert torch.equal(torch.stack([flat[c * F * h * w:c * F * h * w + (fb - fa) * h * w] for c in range(3)]).view(3, fb - fa, h, w), x[:, fa:fb])
