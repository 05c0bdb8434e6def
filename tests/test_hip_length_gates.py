"""-m gpu: one whole UNet evaluation at fp32 accuracy, at every clip length that mixes kernels differently (tests/length_cases.py: one
case per census signature for F = 1..128 at latent side 32 and F = 1..32 at side 64, the shipped architecture with seed-built weights).

Per case, with the model built once for the module:
  * the census of the evaluation that runs -- a thin recording subclass of HipOps asks form_only before each conv / GEMM launch -- equals
    the CPU census of the case (the dry run over the same orchestration): the mix that the case stands for is the mix that ran;
  * the Python host's forward_with_cond_scale(cond_scale = 1) against the float64 oracle of the fixture:
        rel_err(got, y64) <= C_LEN * e32 + FLOOR,   e32 = CPU fp32's own error against y64 (split_gate's gate and error definition),
    instead of the 1e-4 * max(1, |y|) that the full-architecture tests allow (tests/test_hip_fullsize.py): C_LEN and the measured
    ratios stand in length_cases.py and profiles/length_gate_ratios.md;
  * the C evaluator (CtxEvaluator.forward, its own routing code in csrc/dawn_ctx.hip) bit-identical to the Python host on the same clip.

Mixes now held to fp32 accuracy: every signature up to F = 128 (h = 32) / F = 32 (h = 64), among them Winograd at the 8 x 8 level over
fp32 kernels at the 4 x 4 level (F = 28), the resample form turning on with an odd number of 4-frame groups (F = 50), split 1x1 kernels
on some levels only.  Longer clips (F > 128: the signatures of T96 / C2 / C3 above that range) are still held at 1e-4 only.  The temporal
and attention kernel selectors are not in the census (no dry-run query): which of those kernels ran is not asserted here."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import length_cases as L
from split_gate import FLOOR, fp32_gate_e32
from test_hip_ops import LOG
import dawn_pytorch_amd as D
from dawn_pytorch_amd.ops import HipOps

pytestmark = pytest.mark.gpu


class RecordingOps(L.Census, HipOps):
    """HipOps that records the census of what it launches: before each conv_gemm launch it asks form_only (both queries) of exactly
    that call; ln_inline_ok / split_gemm_ok are recorded by the Census mixin."""

    def __init__(self):
        super().__init__()
        self.census = []

    def conv_gemm(self, in0, w, N, **kw):
        if kw.get("form_only"):
            return super().conv_gemm(in0, w, N, **kw)
        if kw.get("out") is None:        # (one output for the queries and the launch: the descriptor holds its address and stride)
            kw["out"] = self.empty(kw["F"] * (kw.get("Ho") or kw["Hi"]) * (kw.get("Wo") or kw["Wi"]), N, like=in0)
        form3, form1 = super().conv_gemm(in0, w, N, form_only=True, **kw)
        direct = super().conv_gemm(in0, w, N, form_only="direct", **kw)
        in1 = kw.get("in1")
        self.record_conv(kw.get("KH", 1), kw["Hi"], in0.shape[1] + (0 if in1 is None else in1.shape[1]), N, kw.get("mode", 0), form3, form1, direct)
        return super().conv_gemm(in0, w, N, **kw)


@pytest.fixture(scope="module")
def model():
    unet = D.DynamicNfUnet3D(default_num_frames=8, **L.KW, init_seed=0)
    wsum = L.checksum(unet.state_dict().values())
    unet = unet.cuda()
    unet.ops = RecordingOps()
    return unet, wsum


@pytest.mark.parametrize("F,h,t", L.CASES, ids=[L.case_name(F, h) for F, h, _ in L.CASES])
def test_length_gate(F, h, t, model):
    unet, wsum = model
    g = load_golden(L.fixture_name(F, h))
    assert (int(g["T"]), int(g["h"]), int(g["time"])) == (F, h, t)
    np.testing.assert_allclose(wsum, g["weights_checksum"], rtol=1e-12, err_msg="deterministic init differs from the fixture's")
    x, cond, isum = L.clip(F, h)
    np.testing.assert_allclose(isum, g["inputs_checksum"], rtol=1e-12)
    fr = torch.from_numpy(g["frames"]).long()
    y64, e32 = torch.from_numpy(g["y64"]), float(g["e32"])
    name = L.case_name(F, h)

    unet.update_num_frames(F)
    xg, cg = x.cuda(), cond.cuda()
    unet.ops.census = []
    got = unet.forward_with_cond_scale(xg, torch.tensor([t]).cuda(), cond=cg, cond_scale=1.0)[0]
    live = tuple(unet.ops.census)

    P = unet.packed()
    ev = unet.ctx_evaluator()
    rc, rs = P.rotary_tables(F + 2 * L.WIN)
    clip = ev.prepare_clip(xg[0, 3:, 0].contiguous(), cg[0].contiguous(), rc, rs)
    got_c = ev.forward(clip, xg[0, :3].contiguous(), float(t))

    want = L.census(F, h)
    kept = got.cpu()[:, fr]
    per_frame = (kept.double() - y64).abs().amax(dim=(0, 2, 3)) / y64.abs().max()
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps({"op": f"length_census/{name}", "signature": L.signature_digest(live), "cpu_signature": L.signature_digest(want),
                            "calls": [list(e) for e in live]}) + "\n")
    same_c = torch.equal(got_c, got)
    c = L.C_CASE.get((F, h), L.C_LEN)
    assert torch.isfinite(got).all()
    rec = fp32_gate_e32(f"length/{name}", kept, y64, e32, c=c, floor=FLOOR, signature=L.signature_digest(live),
                        worst_frame=int(fr[int(per_frame.argmax())]), c_host_bit_identical=same_c)
    print(f"{name}: rel err {rec['rel_err']:.3e}, e32 {e32:.3e}, ratio {rec['ratio']:.2f}")
    assert live == want, [(i, a, b) for i, (a, b) in enumerate(zip(live, want)) if a != b][:5] or (len(live), len(want))
    assert same_c, float((got_c - got).abs().max())
