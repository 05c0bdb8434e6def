"""The LDS bank model of the window-tiled temporal layer (tools/tl16_lds_banks.cpp), built with the host compiler and run: the sites
re-laid for it -- the bias-table reads and the V^T fragment reads -- are predicted conflict-free, for both kernels and at the
benchmark's and the tests' shapes; and the byte offsets the program takes from csrc/temporal_layer16.h (the ones the kernels use) are
those of the layouts the header documents, for a sample of lanes."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "dawn-pytorch_amd", "csrc")
SHAPES = [(200, 0, 200, 40, 4096), (200, 0, 200, 8, 4), (208, 40, 128, 40, 4), (17, 0, 17, 8, 4), (200, 47, 120, 40, 4), (96, 0, 96, 40, 4)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tl16_lds_banks") / "tl16_lds_banks")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tools", "tl16_lds_banks.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def sites(out):
    """{(layout, waves, shape, site): (accesses, LDS cycles conflict-free, extra cycles)} of the SITE lines."""
    got = {}
    for m in re.finditer(r'^SITE (\w+) (\d+) ([\d:]+) "([^"]+)" (\d+) (\d+) (\d+)$', out, re.M):
        got[(m.group(1), int(m.group(2)), m.group(3), m.group(4))] = tuple(int(m.group(i)) for i in (5, 6, 7))
    return got


def test_relaid_sites_are_predicted_conflict_free(prog):
    args = []
    for s in SHAPES:
        args += ["--shape", *s]
    got = sites(run(prog, *args))
    for Fext, q0, Fq, win, _ in SHAPES:
        shape = f"{Fext}:{q0}:{Fq}:{win}"
        for waves in (13, 8):
            for site in ("bias table: read", "V^T: read", "bias table: store", "V^T: store", "K planes: read", "X planes: read, K/V projection"):
                n, _, extra = got[("current", waves, shape, site)]
                assert n > 0 and extra == 0, (shape, waves, site, n, extra)
    # what the change removed, at the benchmark's level-0 shape: the parent's bias-table reads carried 8 extra cycles each, and its V^T
    # fragments took twice the LDS cycles (one ds_read2_b64 = 8 against two ds_read_b64 = 4)
    lvl0 = "200:0:200:40"
    n, _, extra = got[("parent", 13, lvl0, "bias table: read")]
    assert extra == 8 * n
    assert got[("parent", 13, lvl0, "V^T: read")][1] == 2 * got[("current", 13, lvl0, "V^T: read")][1]
    # and what it left: the phase-0 stores (8-way) and the K-plane stores (2-way), unchanged
    for site in ("X planes: store (phase 0)", "K planes: store"):
        assert got[("current", 13, lvl0, site)] == got[("parent", 13, lvl0, site)] and got[("current", 13, lvl0, site)][2] > 0


def header_int(name):
    text = open(os.path.join(CSRC, "temporal_layer16.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_program_offsets_are_the_documented_layouts(prog):
    rows, stride, lds = header_int("TL16_ROWS"), header_int("TL16_BAND_STRIDE"), header_int("TL16_LDS_BYTES")
    nb = rows // 16
    xb, kb = 3 * 8 * rows * 16, 3 * 4 * rows * 16
    vb = 3 * nb * 2 * 512
    assert xb + kb + vb + 4 * header_int("TL16_BAND_ROOM") * 4 == lds
    seen = set()
    for m in re.finditer(r"^OFF (\w+) (\d+) (\d+) (\d+) (\d+) (\d+)$", run(prog, "--offsets"), re.M):
        kind, (a, b, c, d, off) = m.group(1), map(int, m.groups()[1:])
        seen.add(kind)
        if kind == "x":        # [plane][channel octet][row] x 16 B, 8-byte halves
            want = ((a * 8 + b) * rows + c) * 16 + d * 8
        elif kind == "k":      # after the X planes: [plane][k-group][row] x 16 B
            want = xb + ((a * 4 + b) * rows + c) * 16 + d * 8
        elif kind == "v":      # then V^T: [plane][m-block][lane][row block] x 8 B
            want = xb + kb + (((a * 2 + b) * 64 + c) * nb + d) * 8
        else:                  # then the bias table: lane (query n, k-group g), slot: copy (15 - n) & 3, entries 15 - n + 4 g + 16 slot + r
            n, g, blk = a, b, c
            sh = (15 - n) & 3
            want = xb + kb + vb + 4 * (sh * stride + (15 - n - sh) + 4 * g + 16 * blk)
            assert off % 16 == 0 and want + 16 <= lds
        assert off == want, (m.group(0), want)
    assert seen == {"x", "k", "v", "band"}
