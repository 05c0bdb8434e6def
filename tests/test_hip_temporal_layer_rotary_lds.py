"""-m gpu: the window-tiled fused temporal layer (csrc/temporal_layer16.hip) with tables no real clip has: rotary cos / sin that are
independent random numbers per (row, feature pair) and a random per-head bias band.  The kernels keep a wave's query-side rotary rows
across the eight heads and read the bias table through shifted copies; with random tables a value taken from the wrong row, feature
block, head or table copy changes the result (with real tables neighbouring rows differ by a small rotation and could hide it).

Every case runs through the default kernel (13 waves, one query tile each) and the 8-wave kernel (WMODE 4: one query tile per wave up
to 8 tiles, two above -- the 200-row case), against the oracle op set at the tolerance of
test_hip_ops.test_temporal_layer_c64 (3e-5 of max(1, max|ref|): split-bf16 contractions are fp32-accurate, the difference is summation
order), and four runs must be bit-identical."""
import pytest
import torch

from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
from dawn_pytorch_amd.policy import TemporalFlags as TF
from test_hip_ops import check, gpu, hip, packw, ref, rnd  # noqa: F401  (hip / ref: fixtures)

pytestmark = pytest.mark.gpu

HW = 4
# Fext, q0, Fq: one tile with clamped rows; a 1-row second tile; six key blocks with an untrimmed middle; 13 tiles (the benchmark's
# row count); halo rows on both sides (the shard shape: q0 - win is a multiple of 16 at both windows, delta = 0); the same with the
# query range 7 rows off the 16-row grid (delta = 7: the first tile starts before q0, its first rows are not stored)
SHAPES = [(16, 0, 16), (17, 0, 17), (96, 0, 96), (200, 0, 200), (208, 40, 128), (200, 47, 120)]
FLAGS = ((0, "default_13_waves"), (TF.force_wmode(4), "wmode4_8_waves"))
_cache = {}


def _case(ref, Fext, q0, Fq, win):
    key = (Fext, q0, Fq, win)
    if key not in _cache:
        x = rnd(Fext * HW, 64, seed=21) * 1.3 + 0.2
        wqkv, wout = packw(64, 768, seed=22), packw(256, 64, seed=23)
        g = torch.Generator().manual_seed(24 + Fext + win)
        rc, rs = torch.rand(Fext, 16, generator=g) * 2 - 1, torch.rand(Fext, 16, generator=g) * 2 - 1   # in [-1, 1) like cos / sin
        band = rnd(2 * win + 1, 8, seed=25)
        want = ref.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band)
        kw = dict(wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda(), wout_bf3p=pack_bf3_temporal_out(unpack_kn(wout)).cuda())
        _cache[key] = (gpu(x, wqkv, wout, rc, rs, band), kw, want)
    return _cache[key]


@pytest.mark.parametrize("flags,name", FLAGS, ids=[n for _, n in FLAGS])
@pytest.mark.parametrize("win", [8, 40])
@pytest.mark.parametrize("Fext,q0,Fq", SHAPES)
def test_temporal_layer_random_rotary_and_band(hip, ref, Fext, q0, Fq, win, flags, name):
    (x, wqkv, wout, rc, rs, band), kw, want = _case(ref, Fext, q0, Fq, win)
    try:
        hip.temporal_flags = flags
        first = hip.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band, **kw)
        check(f"temporal_layer_random_tables_{name}/F{Fext}_q{q0}_{Fq}_w{win}", first, want, 3e-5)
        for rep in range(3):
            again = hip.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band, **kw)
            assert torch.equal(again, first), f"{name}: run {rep + 1} differs from run 0 in {int((again != first).sum())} elements"
    finally:
        hip.temporal_flags = 0
