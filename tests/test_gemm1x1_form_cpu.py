"""dawn_gemm1x1_form (include/dawn_hip.h): which split-operand kernel dawn_conv_gemm runs a 1x1 projection or a 4x4 / stride-2 resample on.
The answer is the launch's own routing run dry (split1x1_form in csrc/conv_gemm.hip), so the GPU precision gates can assert which kernel they
measure.  No GPU: nothing is launched, the pointers are never dereferenced."""
import ctypes as C

import pytest

from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.policy import ConvPolicy as CP

NONE, TILED, ROWREG, ROWACC, RESAMPLE = 0, 1, 2, 3, 4
DEFAULT, FAKE = 0, 0x1000          # policy 0 = the shipped default; FAKE = any non-null 16-byte aligned "device pointer"


def desc(M=51200, N=768, C0=128, C1=0, bf3=True, policy=DEFAULT, ln=False, row_stats=False, res=False, ld0=None, down=False, up=False,
         tr=False, gn=False):
    d = _lib.ConvDesc()
    d.in0, d.C0, d.ld0 = FAKE, C0, C0 if ld0 is None else ld0
    if C1:
        d.in1, d.C1, d.ld1 = FAKE, C1, C1
    if down:                       # M output rows of 16 x 16 pixels from 32 x 32 inputs
        d.F, d.Hi, d.Wi, d.Ho, d.Wo, d.KH, d.KW, d.stride, d.pad = M // 256, 32, 32, 16, 16, 4, 4, 2, 1
    elif up:                       # M input rows of 16 x 16 pixels -> 32 x 32 outputs, four 2 x 2 phases
        d.F, d.Hi, d.Wi, d.Ho, d.Wo, d.KH, d.KW, d.stride, d.mode = M // 256, 16, 16, 32, 32, 2, 2, 1, 1
    else:
        d.F, d.Hi, d.Wi, d.Ho, d.Wo, d.KH, d.KW, d.stride = M // 256, 16, 16, 16, 16, 1, 1, 1
    d.w, d.N, d.out, d.ld_out = FAKE, N, FAKE, N
    if bf3:
        d.w_bf3 = FAKE
    if ln:
        d.ln_eps = 1e-5
    if row_stats:
        d.row_mean, d.row_rstd = FAKE, FAKE
    if res:
        d.res, d.ld_res = FAKE, N
    if tr:
        d.tr, d.ld_tr, d.tr_a, d.tr_b = FAKE, N, FAKE, FAKE
    if gn:
        d.gn_part = FAKE
    d.policy = policy
    return d


def form(d):
    return _lib.lib().dawn_gemm1x1_form(C.byref(d))


@pytest.mark.parametrize("kw,want", [
    # the production shapes of the precision gates (profiles/r6_insitu_shapes.txt, r6_config1_insitu_shapes.txt)
    (dict(M=12800, N=768, C0=512, res=True), TILED),                # deepest level's to_qkv-sized GEMM with a residual: 128 x 64 tiles
    (dict(M=51200, N=768, C0=256), TILED),
    (dict(M=51200, N=64, C0=128), ROWREG),                          # K = 128: rows stationary in registers
    (dict(M=51200, N=768, C0=128, ln=True), ROWREG),                # ... with the LayerNorm inside
    (dict(M=51200, N=768, C0=64, C1=64, row_stats=True), ROWREG),
    (dict(M=51200, N=128, C0=256), ROWACC),                         # K >= 256, N <= 192: the row-accumulator kernel
    (dict(M=12800, N=192, C0=512, ln=True), ROWACC),
    (dict(M=12800, N=192, C0=256, C1=256, ln=True), ROWACC),
    (dict(M=51200, N=128, C0=128, down=True), RESAMPLE),            # Downsample 4 x 4 / stride 2
    (dict(M=51200, N=128, C0=128, up=True), RESAMPLE),              # Upsample: 2 x 2 phase taps
    # not split, or not this family
    (dict(bf3=False), NONE),
    (dict(M=51200, N=768, C0=512, ln=True), NONE),                  # LayerNorm inside needs whole rows: dawn_conv_gemm answers -14
    (dict(M=51200, N=64, C0=256), ROWACC),
    (dict(M=51200, N=64, C0=512, C1=512, res=True), ROWACC),
    (dict(M=51200, N=64, C0=96, C1=96), NONE),                      # K = 192: neither row kernel, and N = 64 tiles stay on fp32
    (dict(M=4096, N=768, C0=128), NONE),                            # below the split kernels' smallest M
    (dict(M=51200, N=768, C0=128, ld0=130), NONE),                  # a row stride that is no multiple of 16 bytes
    (dict(M=51200, N=768, C0=128, gn=True), NONE),                  # fused GroupNorm statistics: not in these kernels
    (dict(M=51200, N=128, C0=128, down=True, tr=True), NONE),       # resample with an epilogue it does not have
    (dict(M=51200, N=768, C0=128, policy=CP.TILED_ONLY), TILED),     # NO_ROW_KERNELS: the tiled kernel for every shape
    (dict(M=51200, N=128, C0=128, down=True, policy=CP.TILED_ONLY), NONE),
    (dict(M=51200, N=768, C0=128, policy=CP.DEFAULT & ~CP.SPLIT), NONE),      # split kernels off
    # the M = 6400 / 25600 launch classes of the precision gates (configs[1]'s deepest level; every tile plan of gemm1x1_split_plan).  New
    # descriptors go at the end of the table: a test's id carries its position
    (dict(M=6400, N=768, C0=512, res=True), TILED),                 # 150 wide tiles at M <= 12800: 128 x 64 tiles
    (dict(M=6400, N=512, C0=256), TILED),
    (dict(M=25600, N=128, C0=96), TILED),                           # 100 wide tiles, M > 12800: the 256 x 64 plan
    (dict(M=25600, N=768, C0=256, res=True), TILED),                # 600 wide tiles: the 256 x 128 plan
    (dict(M=6400, N=192, C0=64, ln=True), ROWREG),                  # K = 64
    (dict(M=25600, N=128, C0=64), ROWREG),
    (dict(M=25600, N=192, C0=64, C1=64, ln=True), ROWREG),
    (dict(M=6400, N=192, C0=512, C1=512, ln=True), ROWACC),         # K = 1024 from two sources, the LayerNorm inside
    (dict(M=6400, N=64, C0=256), ROWACC),
    (dict(M=25600, N=128, C0=512), ROWACC),
    (dict(M=12800, N=64, C0=64, down=True), RESAMPLE),              # 64 channels at 32 x 32 -> 16 x 16 (configs[1]'s first pair)
    (dict(M=12800, N=64, C0=64, up=True), RESAMPLE),
])
def test_gemm1x1_form(kw, want):
    assert form(desc(**kw)) == want


def test_form_of_null_is_none():
    assert _lib.lib().dawn_gemm1x1_form(None) == NONE


def test_form_agrees_with_the_split_predicates():
    """dawn_gemm1x1_split_ok / dawn_gemm1x1_ln_inline_ok answer the same question from the shape alone (aligned layout, default policy)."""
    L = _lib.lib()
    for M in (6400, 12800, 51200, 204800):
        for N in (64, 128, 192, 256, 384, 768):
            for C0, C1 in ((64, 0), (128, 0), (64, 64), (256, 0), (512, 0), (256, 256), (512, 512), (96, 0), (160, 128)):
                f = form(desc(M=M, N=N, C0=C0, C1=C1))
                assert (f != NONE) == bool(L.dawn_gemm1x1_split_ok(M, N, C0, C1)), (M, N, C0, C1, f)
                fl = form(desc(M=M, N=N, C0=C0, C1=C1, ln=True))
                assert fl in (NONE, ROWREG, ROWACC)
                assert (fl != NONE) == bool(L.dawn_gemm1x1_ln_inline_ok(M, N, C0, C1)), (M, N, C0, C1, fl)
