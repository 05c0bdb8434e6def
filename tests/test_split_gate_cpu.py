"""The fp32-accuracy gate of tests/split_gate.py can fail: for every gate case, built with the same inputs and weights as the GPU test
(fewer frames; H, W and channels unchanged), it REJECTS the op computed with each weight the kernel splits
  * truncated to its top two bf16 planes (the a1 . b3 term lost), and
  * given the third plane of another matrix (a stale prefetch),
and ACCEPTS the op evaluated in fp32 on CPU.  No GPU."""
import pytest
import torch

from oracle.ops_ref import RefOps
import split_gate as G

CPU_FRAMES = {"gemm": 64, "down": 4, "up": 4, "conv3": 32, "temporal": 280, "temporal_seg": 400, "sla": 2, "xattn": 1}     # (conv3: as on the GPU)


@pytest.mark.parametrize("case", G.CASES, ids=[c.name for c in G.CASES])
def test_gate_rejects_plane_defects(case):
    case = case.with_frames(CPU_FRAMES[case.kind])
    ops = RefOps()
    T, Wkn = case.make()
    want64 = case.ref(ops, T, Wkn, G.torch.float64)
    base32 = case.base32(ops, T, Wkn)
    assert not G.gate_rejects(base32, want64, base32, c=case.c)
    errs = {"fp32": G.rel_err(base32, want64)}
    for defect in (G.drop_third, G.stale_third):
        mut = case.ref(ops, T, case.mutant(Wkn, defect), G.torch.float64)
        errs[defect.__name__] = G.rel_err(mut, want64)
    bound = case.c * errs["fp32"] + G.FLOOR
    assert errs["drop_third"] > bound and errs["stale_third"] > bound, (case.name, bound, errs)


def test_the_gate_itself():
    t = G.torch.linspace(1.0, 2.0, 100, dtype=G.torch.float64)
    base = t.float()
    G.fp32_gate("self", t.float(), t, base, log=False)
    with pytest.raises(AssertionError):
        G.fp32_gate("self", (t * (1 + 3e-6)).float(), t, base, log=False)
    w = G.coherent(G.rnd(64, 96, seed=3) * 0.1)
    w1, w2, w3 = G.planes3(w)
    assert torch.equal(w1.double() + w2.double() + w3.double(), w.double())              # exact in fp32, split back into its planes
    assert bool((w3 * w > 0).all()) and float((w3 / w).min()) > 6e-6                       # third plane maximal, with the weight's sign
    from dawn_pytorch_amd.pack import pack_bf3
    third = pack_bf3(w)[:, 2].view(torch.bfloat16).float()                                # [K/16][2][N][8] -> (K, N)
    assert torch.equal(third.permute(0, 1, 3, 2).reshape(64, 96), w3)                       # ... the plane the kernels read
