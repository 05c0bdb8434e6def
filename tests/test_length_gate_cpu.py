"""CPU side of the clip-length gates (tests/length_cases.py, tests/test_hip_length_gates.py): the census justifies the case table, the
fixtures are those of the cases, the float64 oracle agrees with the reference's own output, and the gate at the chosen C_LEN is tighter
than the 1e-4 it replaces for these lengths, accepts CPU fp32 and is shown against a lost third weight plane."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import length_cases as L
from oracle import dawn_oracle as O
from split_gate import FLOOR, drop_third, rel_err

CENSUS_RANGE = {32: 128, 64: 32}        # h -> the lengths F = 1 .. n whose signatures the cases must cover


def gate_bound(F, h, e32):
    return L.C_CASE.get((F, h), L.C_LEN) * e32 + FLOOR


def test_census_coverage():
    """Every distinct census signature that occurs for F = 1..128 at h = 32 and F = 1..32 at h = 64 is the signature of a case, and no
    two cases share one unless length_cases.SAME_SIGNATURE says what else distinguishes them."""
    by_sig = {}
    for F, h, _ in L.CASES:
        assert F <= CENSUS_RANGE[h]
        by_sig.setdefault((h, L.census(F, h)), []).append((F, h))
    for h, n in CENSUS_RANGE.items():
        missing = {}
        for F in range(1, n + 1):
            if (h, L.census(F, h)) not in by_sig:
                missing.setdefault(L.signature_digest(L.census(F, h)), []).append(F)
        assert not missing, f"h = {h}: signatures without a case, by length: {missing}"
    shared = {tuple(sorted(v)) for v in by_sig.values() if len(v) > 1}
    assert shared == set(L.SAME_SIGNATURE), shared


def test_census_is_the_routers_answers():
    """Spot checks of the census against the thresholds it was read from (F = 28, h = 32: Winograd F(2x2) at the 8 x 8 level, the fp32
    kernels at the 4 x 4 level -- 28 x 16 rows are no multiple of 256 --, split 1x1 kernels on the two upper levels only)."""
    sig = L.census(28, 32)
    conv3 = {(e[1], e[4] != 0 or e[6] != 0) for e in sig if e[0] == "conv3"}
    assert conv3 == {(32, True), (16, True), (8, True), (4, False)}
    assert {e[1] for e in sig if e[0] == "conv1" and e[5] != 0} == {32, 16}
    # the resample form turns on at level 1 from F = 50 (50 x 256 output rows = 12800), not before
    assert [e[5] for e in L.census(50, 32) if e[0] == "conv4"][0] == 4 and [e[5] for e in L.census(48, 32) if e[0] == "conv4"][0] == 0
    assert len(L.census(28, 32)) > 100 and L.census(28, 32) != L.census(29, 32)


@pytest.mark.parametrize("F,h,t", L.CASES, ids=[L.case_name(F, h) for F, h, _ in L.CASES])
def test_fixture_is_the_case(F, h, t):
    g = load_golden(L.fixture_name(F, h))
    assert (int(g["T"]), int(g["h"]), int(g["time"])) == (F, h, t)
    assert g["frames"].tolist() == L.kept_frames(F, h) and g["y64"].shape == (3, len(g["frames"]), h, h) and g["y64"].dtype == np.float64
    np.testing.assert_allclose(L.full_unet()[1], g["weights_checksum"], rtol=1e-12)
    np.testing.assert_allclose(L.clip(F, h)[2], g["inputs_checksum"], rtol=1e-12)
    assert 0 < float(g["e32"]) < 1e-5 and 0 < float(g["e32_all"]) < 1e-5 and int(g["threads"]) >= 1 and str(g["torch_version"])
    # the gate is tighter than the 1e-4 * max(1, |y|max) of the full-architecture tests (a condition, not a measurement)
    ymax = float(np.abs(g["y64"]).max())
    assert gate_bound(F, h, float(g["e32"])) < 1e-4 * max(1.0, ymax) / ymax


def test_kept_frames():
    assert L.kept_frames(40, 32) == list(range(40)) and L.kept_frames(10, 64) == list(range(10))
    assert L.kept_frames(50, 32) == sorted({0, 8, 16, 24, 32, 40, 48} | set(range(33, 50)))      # frame 0, every 8th, the last 17
    assert L.kept_frames(28, 64) == [0, 8, 16, 23, 24, 25, 26, 27]


def test_want64_against_the_reference_fixture():
    """The float64 oracle against the reference's own fp32 output of the same clip (full_T96.npz, produced by running the reference):
    their difference is of the size of e32, CPU fp32's error -- the reference is one more fp32 evaluation, with oneDNN's convolution
    in place of im2col + GEMM.  Bound: 3 x e32 (two independent fp32 evaluations of e32 each would give ~1.4 x; oneDNN's own error at
    long K is up to a few times the GEMM's, split_gate.py).  Measured 1.19e-6 against e32 = 9.68e-7 (ratio 1.22)."""
    F, h, t = 96, 32, 627
    assert (F, h, t) in L.CASES
    g, ref = load_golden(L.fixture_name(F, h)), load_golden("full_T96.npz")
    np.testing.assert_allclose(g["inputs_checksum"], ref["inputs_checksum"], rtol=1e-12)
    np.testing.assert_allclose(g["weights_checksum"], ref["weights_checksum"], rtol=1e-12)
    assert ref["frames"].tolist() == list(range(F))
    d = rel_err(torch.from_numpy(ref["y"])[:, torch.from_numpy(g["frames"])], torch.from_numpy(g["y64"]))
    print(f"reference fp32 vs want64: {d:.3e}, e32 {float(g['e32']):.3e}, ratio {d / float(g['e32']):.2f}")
    assert d <= 3 * float(g["e32"])


def _full_fp64_constants(monkeypatch):
    """The three shared fp32 roundings of oracle.dawn_oracle.unet_forward computed in float64 instead."""
    def rotary_tables(T, dim=O.DIM_HEAD, theta=10000.0, pos0=0):
        freqs = 1.0 / (theta ** (torch.arange(0, dim, 2).double() / dim))
        ang = torch.arange(pos0, pos0 + T).double()[:, None] * freqs[None, :]
        return ang.cos(), ang.sin()

    def sinusoidal_emb(t, dim=64, dtype=torch.float64):
        half = dim // 2
        f = torch.exp(torch.arange(half, dtype=torch.float64) * -(np.log(10000) / (half - 1)))
        e = t.double()[:, None] * f[None, :]
        return torch.cat((e.sin(), e.cos()), dim=-1)

    def rel_pos_bucket(rel, num_buckets=32, max_distance=32):
        n = -rel
        half = num_buckets // 2
        ret = (n < 0).long() * half
        n = n.abs()
        max_exact = half // 2
        large = max_exact + (torch.log(n.double() / max_exact) / np.log(max_distance / max_exact) * (half - max_exact)).long()
        return ret + torch.where(n < max_exact, n, torch.minimum(large, torch.full_like(large, half - 1)))
    for fn in (rotary_tables, sinusoidal_emb, rel_pos_bucket):
        monkeypatch.setattr(O, fn.__name__, fn)


def test_shared_fp32_roundings(monkeypatch):
    """want64 keeps three fp32 roundings that model and kernels share by definition (rotary angles and tables, the sinusoidal argument
    t * f, the band's buckets).  Computed in full float64 instead, want64 moves by the figure printed here.  Measured: 3.43e-7 =
    0.42 x e32 at t = 999 (F = 1), 1.27e-7 = 0.14 x e32 at t = 700 (F = 16), 1.4e-9 = 0.001 x e32 at t = 12 (F = 3): it grows with t,
    through the sinusoidal argument (sin(t * f) itself is off by ~6e-5 at t ~ 1000; the time MLP and the FiLM pass little of that
    on).  Up to half of CPU fp32's whole error, common to the GPU and to CPU fp32: the fixtures keep the fp32 constants, so that the
    gate's margin is not spent on it."""
    move = {}
    for (F, h, t) in ((1, 32, 999), (3, 32, 12), (16, 32, 700)):
        g = load_golden(L.fixture_name(F, h))
        sd = dict(L.full_unet()[0].state_dict())
        x, cond, _ = L.clip(F, h)
        y64 = torch.from_numpy(g["y64"])
        kept = L.oracle(sd, x, cond, t, torch.float64)
        assert kept.dtype == torch.float64 and rel_err(kept, y64) < 1e-12       # the fixture is this oracle's output (BLAS blocking aside)
        with monkeypatch.context() as m:
            _full_fp64_constants(m)
            full = L.oracle(sd, x, cond, t, torch.float64)
        move[(F, h, t)] = rel_err(full, y64) / float(g["e32"])
        print(f"F = {F}, h = {h}, t = {t}: full-fp64 constants move want64 by {rel_err(full, y64):.3e} = {move[(F, h, t)]:.2f} x e32")
    assert all(np.isfinite(v) and v > 0 for v in move.values())


def _mutant(sd, names):
    sd64 = L.cast_sd(sd, torch.float64)
    for k in names:
        sd64[k] = drop_third(sd[k].detach())
    return sd64


# (F, h) -> measured ratio defect / e32 of a lost third weight plane (drop_third on every weight the case's census sends to a split
# kernel) that the gate at C_LEN does NOT reject: test_gate_discrimination asserts that exactly these pass the gate
BELOW_GATE = {
}

SMALLEST_WITH_SPLIT_WEIGHTS = [(1, 32, 999), (3, 32, 12)]


def test_the_two_smallest_cases_with_split_weights():
    with_split = sorted((F * h * h, F, h, t) for F, h, t in L.CASES if L.split_weights(F, h))
    assert [c[1:] for c in with_split[:2]] == SMALLEST_WITH_SPLIT_WEIGHTS


@pytest.mark.parametrize("F,h,t", SMALLEST_WITH_SPLIT_WEIGHTS, ids=[L.case_name(F, h) for F, h, _ in SMALLEST_WITH_SPLIT_WEIGHTS])
def test_gate_discrimination(F, h, t):
    """The gate of tests/test_hip_length_gates.py at the chosen C_LEN, on the two smallest cases whose census sends any weight to a
    split-operand kernel: it accepts the fp32 CPU evaluation, and a float64 evaluation with the third bf16 plane of every such weight
    dropped (split_gate.drop_third) is rejected -- unless the case stands in BELOW_GATE with its measured ratio."""
    g = load_golden(L.fixture_name(F, h))
    y64, e32 = torch.from_numpy(g["y64"]), float(g["e32"])
    sd = dict(L.full_unet()[0].state_dict())
    x, cond, _ = L.clip(F, h)
    bound = gate_bound(F, h, e32)
    y32 = L.oracle(sd, x, cond, t, torch.float32)
    assert rel_err(y32, y64) <= bound, (rel_err(y32, y64), bound)
    names = L.split_weights(F, h)
    assert names
    with torch.no_grad():
        ym = O.unet_forward(_mutant(sd, names), x.double(), torch.tensor([t]), cond.double(), win=L.WIN, p="")[0]
    e = rel_err(ym, y64)
    print(f"{L.case_name(F, h)}: {len(names)} split weights, third plane dropped: {e:.3e} = {e / e32:.2f} x e32; bound {bound:.3e} = "
          f"{bound / e32:.2f} x e32")
    assert (e > bound) == ((F, h) not in BELOW_GATE), (e / e32, bound / e32)
