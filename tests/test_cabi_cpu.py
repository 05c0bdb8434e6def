"""No-GPU checks of the C-ABI library: it loads, exports every symbol include/dawn_hip.h declares, and the
ctypes mirror of `dawn_conv_desc` has the C layout (no compute calls without a GPU)."""
import ctypes
import os
import re

from conftest import ROOT
from dawn_pytorch_amd import _lib


def header_functions():
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L = _lib.lib()
    names = header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/dawn_hip.h but not exported by libdawn_hip.so"
    # whole-path entry points (bound with their own argtypes in dawn_pytorch_amd/ctx.py) + host-side helpers
    CTX = {"dawn_ctx_create", "dawn_ctx_destroy", "dawn_ctx_set_option", "dawn_clip_bytes", "dawn_workspace_bytes",
           "dawn_clip_prepare", "dawn_unet_forward", "dawn_sampler_run", "dawn_ctx_profile_read", "dawn_chw_to_hwc",
           "dawn_rotary_tables", "dawn_rel_pos_bucket", "dawn_workspace_bytes_sharded", "dawn_unet_forward_sharded",
           "dawn_sampler_run_sharded"}
    declared = set(names) - {"dawn_last_error", "dawn_abi_version"} - CTX
    assert CTX <= set(names)
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    assert L.dawn_abi_version() == 8
    # no process-global tuning hooks / ablation entry points in the shipped library (policy travels in dawn_conv_desc)
    for gone in ("dawn_conv_set_variant", "dawn_conv_set_debug"):
        assert not hasattr(L, gone), gone


def test_conv_desc_layout_matches_c():
    """Offsets computed the way a C compiler lays out the struct in the header (natural alignment)."""
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    body = src[src.index("typedef struct dawn_conv_desc {") + 31:src.index("} dawn_conv_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        is_wide = "*" in decl or decl.startswith("size_t") or decl.startswith("double")
        for name in re.sub(r"^(const\s+)?(float|int|double|void|size_t|unsigned)\s*\*?", "", decl).split(","):
            fields.append((name.strip().lstrip("*").strip(), 8 if is_wide else 4))
    off, expect = 0, {}
    for name, size in fields:
        off = (off + size - 1) // size * size
        expect[name] = off
        off += size
    for name, _ in _lib.ConvDesc._fields_:
        assert getattr(_lib.ConvDesc, name).offset == expect[name], name
    assert ctypes.sizeof(_lib.ConvDesc) == (off + 7) // 8 * 8


def test_host_side_helpers_match_python_and_reference():
    """Pure host functions of the C evaluator, callable without a GPU: the relative-position bucket against the
    reference-generated table (tests/golden/tables.npz, MT:92-109) and the split-GEMM dispatch predicate."""
    import numpy as np
    from conftest import load_golden
    L = _lib.lib()
    g = load_golden("tables.npz")
    for rel, b in zip(g["rel"].tolist(), g["bucket"].tolist()):
        assert L.dawn_rel_pos_bucket(int(rel)) == int(b), rel
    # the split-GEMM dispatch predicate is a host function of the library (HipOps asks it, there is no Python mirror)
    want = {(204800, 768, 128, 0): 1, (819200, 64, 64, 64): 1, (12800, 768, 512, 0): 1, (12800, 512, 256, 0): 1, (256, 768, 128, 0): 0,
            (12801, 768, 128, 0): 0, (204800, 768, 48, 0): 0, (819200, 64, 256, 0): 1, (819200, 64, 192, 0): 0, (51200, 192, 256, 256): 1}
    for (M, N, C0, C1), ok in want.items():
        assert int(L.dawn_gemm1x1_split_ok(M, N, C0, C1)) == ok, (M, N, C0, C1)


def test_ctx_structs_match_header():
    """ctypes mirrors of dawn_unet_cfg / dawn_ddim_step have the sizes the C declarations imply."""
    from dawn_pytorch_amd import ctx
    assert ctypes.sizeof(ctx.UnetCfg) == 4 * (2 + 8 + 1 + 3 + 1)
    assert ctypes.sizeof(ctx.DdimStep) == 4 * 7
    assert ctypes.sizeof(ctx.NamedPtr) == 16
    # dawn_shard_comm: void* user; int rank, world; five function pointers
    assert ctypes.sizeof(ctx.ShardCommC) == 8 + 4 + 4 + 5 * 8
    assert ctx.ShardCommC.halo_begin.offset == 16 and ctx.ShardCommC.allreduce_min_u32.offset == 48


def header_constants(prefix):
    """({NAME: value}, {NAME: function}) of include/dawn_hip.h's object-like `#define <prefix>NAME value` (and anonymous-enum
    `<prefix>NAME = value`) and function-like `#define <prefix>NAME(x) (expression in x)` constants, names without the prefix."""
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S).replace("\\\n", " ")
    env = {}            # every DAWN_* constant: a body may name earlier ones (an OR of names, FIELD(15))
    for name, arg, body in re.findall(r"^#define (DAWN_[A-Z0-9_]+)(\(\w+\))?[ \t]+(.+)$", src, flags=re.M):
        env[name] = eval(f"lambda {arg[1:-1]}: {body}" if arg else body, env)          # ((n) << 16), a | b: C and Python agree
    for name, value in re.findall(r"\b(DAWN_[A-Z0-9_]+) *= *(\w+)", src):
        env[name] = eval(value, env)
    mine = {n[len(prefix):]: v for n, v in env.items() if n.startswith(prefix)}
    return ({n: v for n, v in mine.items() if not callable(v)}, {n: v for n, v in mine.items() if callable(v)})


def test_python_names_equal_header_values():
    """policy.ConvPolicy / TemporalFlags / TemporalAttnFlags and ctx.OPT_* are the header's table, name for name and value for value,
    and every named composition is the literal the tests and tools used to spell."""
    from dawn_pytorch_amd import ctx, policy
    CP = policy.ConvPolicy
    compositions = {"FP32_TILES": 0xD, "EXACT_FP32": 0x80D, "HALO_V1": 0x180D, "HALO_V1_NINE": 0x380D, "DIRECT_V2": 0x580D,
                    "DIRECT_V2_NINE": 0x780D, "DIRECT_V2_K32": 0x100580D, "DIRECT_V2_TILE128": 0xD80D, "WINO": 0x300580D,
                    "WINO4_EVERYWHERE": 0x1B00580D, "DEFAULT": 0x2B00580D, "TILED_ONLY": 0x2B02580D}
    for name, value in compositions.items():
        assert int(CP[name]) == value, name
    assert int(CP.DEFAULT) == 0x2B00580D
    default, _ = header_constants("DAWN_CONV_POLICY_")
    assert default == {"DEFAULT": 0x2B00580D}
    for prefix, cls, extra in (("DAWN_POLICY_", CP, set(compositions)), ("DAWN_TL_", policy.TemporalFlags, set()),
                               ("DAWN_TA_", policy.TemporalAttnFlags, set())):
        consts, funcs = header_constants(prefix)
        assert len(consts) >= 4, prefix
        members = {n: int(m) for n, m in cls.__members__.items()}            # (aliases of one bit included)
        assert set(members) - extra == set(consts), (prefix, set(members) - extra ^ set(consts))
        for name, value in consts.items():
            assert members[name] == value, (prefix, name)
        for name, f in funcs.items():                                        # DAWN_POLICY_VARIANT(n) == ConvPolicy.variant(n), ...
            for n in range(6):
                assert int(getattr(cls, name.lower())(n)) == f(n), (prefix, name, n)
    assert set(header_constants("DAWN_POLICY_")[1]) == {"VARIANT", "STAGGER"} and set(header_constants("DAWN_TL_")[1]) == {"FORCE_WMODE"}
    opts, _ = header_constants("DAWN_OPT_")
    assert opts == {n[4:]: getattr(ctx, n) for n in dir(ctx) if n.startswith("OPT_")} and len(opts) == 7


# (file, token) pairs allowed outside dawn_common.h: sites where sharing the definition would have changed device code.  Empty.
SHARED_IDIOM_ALLOW = set()


def test_shared_kernel_idioms_have_one_definition():
    """The truncation mask, the cross-term orders, the buffer-descriptor builtin and the row-sum DPP control are spelled in
    csrc/dawn_common.h and nowhere else in the kernel sources: a change to a split scheme reaches every kernel or none."""
    csrc = os.path.join(ROOT, "dawn-pytorch_amd", "csrc")
    files = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip")))
    files.append(os.path.join(ROOT, "tools", "ubench", "conv3x3_sk.hip"))
    tokens = ("0xffff0000u", "{2, 0, 1, 1, 0, 0}", "{2, 2, 1, 2, 0, 1, 1, 0, 0}", "make_buffer_rsrc", "0x141")
    assert len(files) > 30
    found = set()
    for path in files:
        text = open(path).read()
        found |= {(os.path.basename(path), t) for t in tokens if t in text}
    assert {t for f, t in found if f == "dawn_common.h"} == set(tokens)
    assert {(f, t) for f, t in found if f != "dawn_common.h"} == SHARED_IDIOM_ALLOW
