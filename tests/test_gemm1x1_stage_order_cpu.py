"""The stage wait of gemm1x1_bf16_kernel (`s_waitcnt vmcnt(NQ) lgkmcnt(0)`, csrc/gemm1x1_tiled.hip) lets the NQ youngest memory operations stay in
flight and names them the A rows of the next stage.  That is only true while every stage issues its weight LDS-DMA BEFORE its A-row loads;
a `sched_barrier(0)` between issueB and loadA states it in the source.  This test checks it in the device code of the built object: in the
prologue and in each stage, every LDS-DMA `buffer_load ... lds` precedes every A-row `buffer_load`, and both precede the next stage wait.
No GPU: the code object is disassembled on the host."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


def llvm_bin():
    """The LLVM tools of the ROCm install that builds the library: $ROCM_PATH/llvm/bin, else next to the hipcc on PATH."""
    roots = [os.environ["ROCM_PATH"]] if os.environ.get("ROCM_PATH") else []
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        if os.path.isdir(os.path.join(r, "llvm", "bin")):
            return os.path.join(r, "llvm", "bin")
    return None


OBJ = os.path.join(ROOT, "build", "gemm1x1_tiled.o")
SRC = os.path.join(ROOT, "dawn-pytorch_amd", "csrc", "gemm1x1_tiled.hip")
KERNEL = re.compile(r"_ZN12_GLOBAL__N_119gemm1x1_bf16_kernelILi(\d+)ELi(\d+)ELi(\d+)EEEv14dawn_conv_descl")
STAGE_WAIT = re.compile(r"^s_waitcnt vmcnt\((4|8)\) lgkmcnt\(0\)")
DMA = re.compile(r"^buffer_load_dword\S*\s.*\slds$")
LOAD = re.compile(r"^buffer_load_dword")


def nq(wn, cfg):
    """A quads per thread per stage: BM * 8 / threads (the immediate of the stage wait)."""
    return 4 if cfg else (8 if wn == 1 else 4)


def stage_order_violations(insts, q):
    """Segments of `insts` (prologue, then one per stage wait vmcnt(q)) whose LDS-DMA and A-row loads are out of order."""
    segs, cur = [], []
    for ins in insts:
        if STAGE_WAIT.match(ins) and ins.startswith(f"s_waitcnt vmcnt({q})"):
            segs.append(cur)
            cur = []
        else:
            cur.append(ins)
    segs.append(cur)
    bad = []
    for k, seg in enumerate(segs[:-1]):                # the last segment is the epilogue after the final stage
        dma = [i for i, ins in enumerate(seg) if DMA.match(ins)]
        rows = [i for i, ins in enumerate(seg) if LOAD.match(ins) and not DMA.match(ins)]
        if len(dma) < 3 or len(rows) < q or max(dma) > min(rows):
            bad.append((k, len(dma), len(rows), seg[:40]))
    return len(segs) - 1, bad


def device_code():
    if not os.path.exists(OBJ):
        pytest.skip(f"{os.path.relpath(OBJ, ROOT)} not built (run __graft_entry__.build())")
    if os.path.getmtime(OBJ) < os.path.getmtime(SRC):
        pytest.skip(f"{os.path.relpath(OBJ, ROOT)} is older than its source")
    llvm = llvm_bin()
    tools = [os.path.join(llvm or "", t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if llvm is None or not all(shutil.which(t) for t in tools):
        pytest.skip("needs llvm-objcopy, clang-offload-bundler and llvm-objdump of the ROCm install ($ROCM_PATH or hipcc's)")
    return tools


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    objcopy, bundler, objdump = device_code()
    d = tmp_path_factory.mktemp("isa")
    fb, co = str(d / "conv_gemm.fatbin"), str(d / "conv_gemm.co")
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fb}", OBJ, str(d / "host.o")], check=True)
    subprocess.run([bundler, "--unbundle", "--type=o", f"--input={fb}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                   check=True)
    text = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                          text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\S*\s*<(\S+)>:$", line)
        if m:
            cur = m.group(1) if KERNEL.fullmatch(m.group(1)) else None
            if cur:
                out[cur] = []
        elif cur and line.strip():
            out[cur].append(line.split("//")[0].split(";")[0].strip())
    return out


def test_every_instantiation_is_present(kernels):
    # <NT, WN, CFG>: 6 / 9 cross terms x 256 x 64 / 256 x 128 tiles, and the 128 x 64 two-per-CU tile
    found = {tuple(int(g) for g in KERNEL.fullmatch(k).groups()) for k in kernels}
    assert found == {(6, 1, 0), (6, 2, 0), (9, 1, 0), (9, 2, 0), (6, 1, 1)}, found


def test_weight_dma_precedes_a_rows_in_every_stage(kernels):
    for name, insts in kernels.items():
        nt, wn, cfg = (int(g) for g in KERNEL.fullmatch(name).groups())
        q = nq(wn, cfg)
        nstages, bad = stage_order_violations(insts, q)
        assert nstages >= 2, f"{name}: {nstages} stage waits vmcnt({q}) found"
        assert not bad, f"{name}: weight DMA not ahead of the A rows in segments {[b[:3] for b in bad]}:\n" + "\n".join(bad[0][3])


def test_checker_rejects_a_swapped_stage():
    """The checker itself: the A rows issued ahead of the weight DMA in the second stage is reported."""
    dma = ["buffer_load_dwordx4 v56, s[20:23], s43 offen lds"] * 3
    rows = ["buffer_load_dwordx4 v[2:5], v10, s[44:47], s48 offen"] * 4
    wait = ["s_waitcnt vmcnt(4) lgkmcnt(0)", "s_barrier"]
    good = dma + rows + wait + dma + rows + wait + dma + rows + wait + ["global_store_dwordx4 v[0:1], v[2:5], off"]
    assert stage_order_violations(good, 4) == (3, [])
    swapped = dma + rows + wait + rows + dma + wait + dma + rows + wait
    n, bad = stage_order_violations(swapped, 4)
    assert n == 3 and [b[0] for b in bad] == [1]
