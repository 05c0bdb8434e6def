"""The fp32-accuracy gates of tests/stage_gate.py (HuBERT and PBnet stage kernels) can fail: every case, built with the same inputs as the
GPU test, ACCEPTS the op evaluated in fp32 on the CPU and REJECTS each defect stage_gate lists for it -- a matrix operand truncated to 16
mantissa bits, a lost K chunk, a shifted last row, the neighbouring group's columns, the online softmax without its rescale or without
its tail keys -- emulated in float64 against the same reference and checked with the case's own factor c: a factor widened until a defect
passes fails here.  No GPU."""
import functools

import pytest
import torch

import stage_gate as S

IDS = [c.name for c in S.CASES]


@functools.lru_cache(maxsize=4)
def _refs(name):
    case = next(c for c in S.CASES if c.name == name)
    T = case.make()
    return case, T, case.want64(T), case.base32(T)


def test_case_table_is_the_issue_s():
    """One case per launch / shape the stages run, and the defects each kind must carry."""
    kinds = {}
    for c in S.CASES:
        kinds.setdefault(c.kind, []).append(c)
    assert {k: len(v) for k, v in kinds.items()} == {"hconv": 10, "attn64": 24, "ln": 18, "conv0": 2, "wavenorm": 1, "addact": 2,
                                                     "attn32": 10, "linear": 10}
    assert len(set(IDS)) == len(IDS)
    for c in kinds["hconv"]:
        assert c.defect_names()[:3] == ("precision", "last_chunk_lost", "last_row_shifted")
        assert ("neighbour_group" in c.defect_names()) == (c.p.get("group") is not None)
    assert [c.rows_out() for c in kinds["hconv"]] == [159, 39, 49, 150, 150, 150, 150, 150, 150, 1]
    for c in kinds["attn64"]:          # the exemptions stage_gate's docstring states, and no other
        T = c.p["T"]
        assert ("no_alpha" in c.defect_names()) == (T > 32) and ("tail_keys_lost" in c.defect_names()) == (T in (33, 65, 999, 1000))
    for k in ("attn64", "attn32", "linear", "conv0"):
        assert all("precision" in c.defect_names() for c in kinds[k])
    assert all(c.c >= S.C_GATE for c in S.CASES)


@pytest.mark.parametrize("name", IDS)
def test_gate_accepts_cpu_fp32_and_rejects_defects(name):
    case, T, want64, base32 = _refs(name)
    assert want64.dtype == torch.float64 and base32.dtype == torch.float32 and want64.shape == base32.shape
    assert not S.gate_rejects(base32, want64, base32, c=case.c)
    e32 = S.rel_err(base32, want64)
    bound = case.c * e32 + S.FLOOR
    # the baseline is an fp32 computation: never past fp32 accuracy (at score std 9 a score of ~40 carries 40 x 2^-24 = 2.4e-6 into the
    # exponent; everything else stays below 2e-6); exactly 0 only where the op copies one value (one key: out = v)
    assert e32 < (1e-5 if case.kind in ("attn64", "attn32") else 2e-6), e32
    if not (case.kind == "attn64" and case.p["T"] == 1):
        assert e32 > 1e-9, e32
    errs = {n: S.rel_err(t, want64) for n, t in case.defects(T, want64).items()}
    assert tuple(errs) == case.defect_names()
    kept = {n: e for n, e in errs.items() if not e > bound}
    assert not kept, (case.name, f"bound {bound:.3e} (fp32 {e32:.3e}, c {case.c})", errs)


HOOKED = [c for c in S.CASES if c.kind in ("attn64", "attn32")]


@pytest.mark.parametrize("case", HOOKED, ids=[c.name for c in HOOKED])
def test_hooked_reference_is_the_oracle(case):
    """Without hooks, the hooked float64 copies of attn64 / attn_bias32 are the RefOps ops in float64."""
    case, T, want64, _ = _refs(case.name)
    if case.kind == "attn64":
        got = S.attn64_64(T["qkv"], S.HEADS64)
    else:
        q, k, v = case.qkv32(T["qkv"])
        got = S.attn32_64(q, k, v, S.HEADS32, T["bias"], T["rc"], T["rs"], 32 ** -0.5)
    assert got.dtype == torch.float64 and float((got - want64).abs().max() / want64.abs().max()) <= 1e-14


def test_trunc16_is_the_tf32_class_defect():
    x = S.rnd(4096, seed=5)
    t = S.trunc16(x)
    rel = ((x.double() - t) / x.double()).abs()
    assert bool((t.abs() <= x.double().abs()).all()) and float(rel.max()) < 2.0 ** -15 and float(rel.mean()) > 2.0 ** -19
    assert torch.equal(t.float().double(), t)                       # still a float32 value

