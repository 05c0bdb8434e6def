"""No-GPU checks of the C-ABI library and of its binding: the header reader (dawn_pytorch_amd/abi.py) reads every declaration of
include/dawn_hip.h and refuses what it cannot read, the library exports and binds all of them, and every hand-written ctypes struct
mirror has the header's layout (no compute calls without a GPU)."""
import ctypes
import importlib.util
import os
import re

import pytest

from conftest import ROOT
from dawn_pytorch_amd import _lib, abi


def header_functions():
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src)))


def header_text():
    return open(os.path.join(ROOT, "include", "dawn_hip.h")).read()


def test_library_exports_every_declared_symbol():
    """Every declaration is bound: the names a loose regex finds in the header, the names abi.functions() reads, and the names the
    library exports with the derived argtypes set are one set."""
    L = _lib.lib()
    names = header_functions()
    assert len(names) >= 160
    derived = abi.functions(header_text())
    assert set(names) == set(derived) == set(_lib.SIGNATURES), set(names) ^ set(derived) ^ set(_lib.SIGNATURES)
    for n, (restype, argtypes) in derived.items():
        assert hasattr(L, n), f"{n} declared in include/dawn_hip.h but not exported by libdawn_hip.so"
        fn = getattr(L, n)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes == _lib.SIGNATURES[n] and fn.restype is restype, n
    assert L.dawn_abi_version() == 8 == abi.defines(header_text())["DAWN_ABI_VERSION"]
    # no process-global tuning hooks / ablation entry points in the shipped library (policy travels in dawn_conv_desc)
    for gone in ("dawn_conv_set_variant", "dawn_conv_set_debug"):
        assert not hasattr(L, gone), gone


_p, _i, _l, _f, _d, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
# written out from include/dawn_hip.h by hand: every scalar kind and every return kind appears
PINNED = {
    "dawn_heads_eps": (_i, [_p] * 7 + [_i, _i, _p, _i, _i, _p, _p, _p, _p, _l, _i, _p, _p]),
    "dawn_select_scan": (_i, [_p, _i, ctypes.c_ulonglong, _p, _i, _p]),
    "dawn_philox_normal": (_i, [_p, _i, _i, _i, _i, _i, ctypes.c_uint64, ctypes.c_uint32, _p]),
    "dawn_frames_to_u8": (_i, [_p, _l, _l, _d, _d, _d, _i, _p, _p]),
    "dawn_gn_finalize": (_i, [_p, _d, _p, _p, _p, _p, _i, _f, _p, _p, _p]),
    "dawn_bundle_open": (_i, [ctypes.c_char_p, _p]),
    "dawn_sampler_run_dpmpp": (_i, [_p, _i, _i, _i, _p, _p, _f, _p, _i, _p, _p, _p, _p, _z, _p, _p, _p]),
    "dawn_resample16k_len": (_l, [_l, _i]),
    "dawn_clip_bytes": (_z, [_p, _i, _i, _i]),
    "dawn_ctx_destroy": (None, [_p]),
    "dawn_last_error": (ctypes.c_char_p, []),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    fn = getattr(_lib.lib(), name)
    restype, argtypes = PINNED[name]
    assert fn.restype is restype and list(fn.argtypes) == argtypes


@pytest.mark.parametrize("decl,quoted", [
    ("int dawn_ok(int a);\nint dawn_x(flaot y, void* stream);", "dawn_x(flaot y"),                      # unknown type
    ("int dawn_x(int (*cb)(void* user), void* stream);", "dawn_x(int (*cb)"),                           # function-pointer argument
    ("int dawn_x(int n, ...);", "dawn_x(int n, ...)"),                                                  # outside the grammar
    ("int dawn_x(int);", "dawn_x(int)"),                                                                # unnamed argument
    ("static inline int dawn_x(int n) { return n; }\nint dawn_y(int n);", "dawn_x(int n)"),             # a body, not a declaration
    ("typedef struct dawn_s { int n[DAWN_NOT_DEFINED]; } dawn_s;", "DAWN_NOT_DEFINED"),
    ("typedef struct dawn_s { dawn_other o; } dawn_s;", "dawn_other"),
    ("int dawn_x(int n)", "dawn_x(int n)"),                                                             # no terminating semicolon
])
def test_reader_refuses_what_it_cannot_read(decl, quoted):
    with pytest.raises(abi.HeaderError) as e:
        abi.functions(decl)
    assert quoted in str(e.value)


def test_reader_on_header_strings():
    text = """#define DAWN_N 3  /* a size */
    typedef struct dawn_h dawn_h;
    typedef struct dawn_in { int kind; double q; } dawn_in;
    typedef struct dawn_s { const float* a, * b; int n[DAWN_N], m; dawn_in in; int (*cb)(void* user, int n); const char* name; } dawn_s;
    enum { DAWN_A = 0, DAWN_B = 1 };
    void dawn_f(dawn_h* h, const dawn_s* s, const float* const* rows, unsigned char* bytes, int16_t v, /* comment, with ( */ unsigned u);
    const char* dawn_g(void);   // trailing
    dawn_h* dawn_make(size_t n);"""
    f, s = abi.functions(text), abi.structs(text)
    assert f == {"dawn_f": (None, [_p, _p, _p, _p, ctypes.c_int16, ctypes.c_uint]), "dawn_g": (ctypes.c_char_p, []), "dawn_make": (_p, [_z])}
    assert [n for n, _ in s["dawn_s"]] == ["a", "b", "n", "m", "in", "cb", "name"] and abi.defines(text) == {"DAWN_N": 3}
    S = type("S", (ctypes.Structure,), {"_fields_": s["dawn_s"]})
    assert (S.n.offset, S.m.offset, getattr(S, "in").offset, S.cb.offset, S.name.offset, ctypes.sizeof(S)) == (16, 28, 32, 48, 56, 64)
    assert s["dawn_s"][6][1] is ctypes.c_char_p and s["dawn_s"][0][1] is _p


def test_lib_refuses_a_missing_header_and_another_abi_number(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", tmp_path / "absent.h")
    with pytest.raises(_lib.DawnHipError, match="absent.h"):
        _lib.lib()
    newer = tmp_path / "dawn_hip.h"
    newer.write_text(header_text().replace("#define DAWN_ABI_VERSION 8", "#define DAWN_ABI_VERSION 9"))
    monkeypatch.setattr(_lib, "HEADER_PATH", newer)
    with pytest.raises(_lib.DawnHipError, match=r"ABI version 8.*DAWN_ABI_VERSION 9"):
        _lib.lib()
    # DAWN_HIP_HEADER names the header as DAWN_HIP_LIB names the library; importing the module never fails, lib() does
    monkeypatch.setenv("DAWN_HIP_HEADER", str(tmp_path / "absent.h"))
    spec = importlib.util.spec_from_file_location("dawn_pytorch_amd._lib_without_header", _lib.__file__)
    probe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(probe)
    assert probe.SIGNATURES == {} and len(_lib.SIGNATURES) >= 160
    with pytest.raises(probe.DawnHipError, match="absent.h"):
        probe.lib()


def struct_mirrors():
    from dawn_pytorch_amd import bundle, ctx
    from test_tl16_schedule_cpu import Sched
    return {"dawn_conv_desc": _lib.ConvDesc, "dawn_tl16_sched": Sched, "dawn_unet_cfg": ctx.UnetCfg, "dawn_named_ptr": ctx.NamedPtr,
            "dawn_ddim_step": ctx.DdimStep, "dawn_shard_comm": ctx.ShardCommC, "dawn_ancestral_step": ctx.AncestralStep,
            "dawn_clip_mode": ctx.ClipMode, "dawn_dpmpp_step": ctx.DpmppStep, "dawn_decoder_cfg": ctx.DecoderCfg,
            "dawn_hubert_cfg": ctx.HubertCfg, "dawn_pbnet_cfg": ctx.PbnetCfg, "dawn_inputs_cfg": ctx.InputsCfg,
            "dawn_generate_args": ctx.GenerateArgs, "dawn_media_args": ctx.MediaArgs, "dawn_motion_cfg": ctx.MotionCfg,
            "dawn_reenact_args": ctx.ReenactArgs, "dawn_bundle_defaults": bundle.Defaults}


STRUCTS = sorted(abi.structs(header_text()))


def test_every_header_struct_has_one_mirror():
    from dawn_pytorch_amd import bundle, ctx
    assert STRUCTS == sorted(struct_mirrors()) and len(STRUCTS) == 18
    assert dict(bundle.Defaults._fields_)["clip"] is ctx.ClipMode and not hasattr(bundle, "ClipModeC")


@pytest.mark.parametrize("name", STRUCTS)
def test_struct_mirror_matches_header(name):
    """The hand-written ctypes mirror against the header's struct in natural C layout: field names in order, every offset, every
    field size, sizeof and alignment.  (The C side pins the same layouts with static_asserts; this is the Python side.)"""
    mirror = struct_mirrors()[name]
    want = type(name, (ctypes.Structure,), {"_fields_": abi.structs(header_text())[name]})
    assert [n for n, _ in mirror._fields_] == [n for n, _ in want._fields_]
    for n, _ in want._fields_:
        assert (getattr(mirror, n).offset, getattr(mirror, n).size) == (getattr(want, n).offset, getattr(want, n).size), n
    assert (ctypes.sizeof(mirror), ctypes.alignment(mirror)) == (ctypes.sizeof(want), ctypes.alignment(want))


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
