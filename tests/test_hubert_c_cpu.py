"""No-GPU checks of the C-side HuBERT stage (include/dawn_hip.h: dawn_hubert_*; csrc/dawn_hubert.hip): the entries are exported and
bound, the ctypes mirror of `dawn_hubert_cfg` has the C layout, `dawn_hubert_create` accepts the table HubertFeatures builds and names
the entry it misses, and the pure host functions (conv length, segment plan, workspace size) agree with the Python bookkeeping of
dawn-pytorch_amd/hubert.py.  Nothing is launched: the weight pointers are dummies."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from dawn_pytorch_amd import _lib, ctx
from dawn_pytorch_amd.hubert import HubertFeatures
from oracle.ops_ref import RefOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dawn_hubert_pos_conv", "dawn_hubert_create", "dawn_hubert_destroy", "dawn_hubert_conv_frames", "dawn_hubert_segments",
       "dawn_hubert_workspace_bytes", "dawn_hubert_encode", "dawn_hubert_features")


@pytest.fixture(scope="module")
def tiny():
    g = load_golden("hubert_tiny.npz")
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")}
    return g, HubertFeatures(sd, "cpu", num_heads=int(g["num_heads"]), pos_groups=int(g["pos_groups"]), ops=RefOps())


def large_cfg(layers=24):
    """hubert-large-ls960-ft."""
    cfg = ctx.HubertCfg()
    cfg.n_conv = 7
    for i, (k, s) in enumerate(zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2))):
        cfg.conv_k[i], cfg.conv_stride[i] = k, s
    cfg.conv_dim, cfg.hidden, cfg.heads, cfg.intermediate, cfg.n_layers = 512, 1024, 16, 4096, layers
    cfg.pos_k, cfg.pos_groups, cfg.eps = 128, 16, 1e-5
    return cfg


def names_of(cfg):
    """The weight names include/dawn_hip.h lists for this topology."""
    out = [f"conv.{i}.{f}" for i in range(cfg.n_conv) for f in ("w", "b", "g", "be")]
    out += ["fp.g", "fp.b", "fp.w", "fp.bias", "pos.w", "pos.b", "enc_ln.g", "enc_ln.b"]
    out += [f"layers.{i}.{f}" for i in range(cfg.n_layers)
            for f in ("ln1.g", "ln1.b", "wqkv", "bqkv", "wo", "bo", "ln2.g", "ln2.b", "w1", "b1", "w2", "b2")]
    return out


def create(cfg, names):
    """dawn_hubert_create with dummy non-null pointers -> (rc, handle)."""
    L = _lib.lib()
    arr = (ctx.NamedPtr * max(1, len(names)))()
    keep = [n.encode() for n in names]
    for i, n in enumerate(keep):
        arr[i].name, arr[i].ptr = n, 0x1000 + 256 * i
    h = C.c_void_p()
    rc = L.dawn_hubert_create(C.addressof(cfg), C.addressof(arr), len(names), C.addressof(h))
    return rc, h


@pytest.fixture(scope="module")
def large():
    rc, h = create(large_cfg(), names_of(large_cfg()))
    assert rc == 0 and h.value, _lib.lib().dawn_last_error().decode()
    yield h
    _lib.lib().dawn_hubert_destroy(h)


def test_entries_exported_bound_and_abi_unchanged():
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", src), f"{n} not declared in include/dawn_hip.h"
        assert hasattr(L, n), f"{n} not exported by libdawn_hip.so"
        assert n in _lib.SIGNATURES, f"{n} not bound in _lib.SIGNATURES"
    assert L.dawn_abi_version() == 8
    assert L.dawn_hubert_conv_frames.restype is C.c_long and L.dawn_hubert_workspace_bytes.restype is C.c_size_t


def test_cfg_layout_matches_header():
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    body = src[src.index("typedef struct dawn_hubert_cfg {") + 32:src.index("} dawn_hubert_cfg;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for name in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", name)
            fields.append((m.group(1), ty, int(m.group(2) or 1)))
    assert [f[0] for f in fields] == [f[0] for f in ctx.HubertCfg._fields_]
    assert all(ty in ("int", "float") for _, ty, _ in fields)
    assert C.sizeof(ctx.HubertCfg) == 4 * sum(n for _, _, n in fields) == 100
    for (name, ty, n), (_, cty) in zip(fields, ctx.HubertCfg._fields_):
        assert C.sizeof(cty) == 4 * n and (cty is C.c_float) == (ty == "float"), name


def test_create_accepts_the_python_table_and_names_what_is_missing(tiny):
    L = _lib.lib()
    _, hf = tiny
    cfg, table = ctx.hubert_cfg(hf), ctx.hubert_named_weights(hf)
    assert set(table) == set(names_of(cfg))                       # the names HubertFeatures builds = the names the header lists
    assert tuple(table["pos.w"].shape) == (hf.pos_groups, hf.pos_k * 64 // 4, 64, 4) and table["pos.w"].is_contiguous()
    assert all(torch.equal(table["pos.w"][g], hf.pos_w[g]) for g in range(hf.pos_groups))
    rc, h = create(cfg, list(table))
    assert rc == 0 and h.value, L.dawn_last_error().decode()
    L.dawn_hubert_destroy(h)
    for gone in ("layers.1.w2", "pos.w", "conv.3.be", "enc_ln.b"):
        h0 = C.c_void_p()
        rc, h = create(cfg, [n for n in table if n != gone])
        assert rc != 0 and not h.value and f"'{gone}'" in L.dawn_last_error().decode(), (gone, L.dawn_last_error().decode())
        assert not h0.value
    rc, h = create(cfg, [n for n in table if not re.fullmatch(r"conv\.\d\.b", n)])      # conv_bias = False models: optional
    assert rc == 0
    L.dawn_hubert_destroy(h)


def test_create_refuses_unusable_sizes():
    L = _lib.lib()
    for edit, word in ((dict(heads=15), "64 * heads"), (dict(hidden=1088, heads=17), "gw % 16"), (dict(pos_groups=3), "gw % 16"),
                       (dict(pos_k=1024), "64 KB"), (dict(n_conv=9), "n_conv"), (dict(conv_dim=510), "conv_dim")):
        cfg = large_cfg(2)
        for k, v in edit.items():
            setattr(cfg, k, v)
        rc, h = create(cfg, names_of(large_cfg(2)))
        assert rc != 0 and not h.value and word in L.dawn_last_error().decode(), (edit, L.dawn_last_error().decode())


# ---- the Python bookkeeping of hubert.py, as plain integers
def py_conv_frames(n, ks=(10, 3, 3, 3, 3, 2, 2), st=(5, 2, 2, 2, 2, 2, 2)):
    T = n
    for k, s in zip(ks, st):
        T = (T - k) // s + 1
    return T


def py_plan(n):
    """The loop of HubertFeatures.get_hubert_from_16k_speech + interpolate_25fps on lengths only."""
    kernel, stride = 400, 320
    clip_length = stride * 1000
    num_iter = n // clip_length
    expected_T = (n - (kernel - stride)) // stride
    segs = []
    for i in range(num_iter):
        start = clip_length * i
        segs.append((start, len(range(n)[start:start + (clip_length - stride + kernel)])))
    last = range(n)[clip_length * num_iter:] if num_iter > 0 else range(n)
    if len(last) >= kernel:
        segs.append((clip_length * num_iter if num_iter > 0 else 0, len(last)))
    segs = [(s, ln, py_conv_frames(ln)) for s, ln in segs]
    assert abs(sum(r for _, _, r in segs) - expected_T) <= 1
    num_frames = int((n / 16000) * 25)
    assert len(np.linspace(0, expected_T - 1, num_frames)) == num_frames
    return segs, expected_T, num_frames


def counts(tiny):
    return [400, 32037, 319999, 320000, 320079, 320080, 320399, 320400, 640000, int(tiny[0]["speech"].shape[0])]


def c_plan(h, n, room=16):
    buf, eT, nf = (C.c_long * (3 * room))(), C.c_long(-1), C.c_long(-1)
    ns = _lib.lib().dawn_hubert_segments(h, n, buf, room, C.byref(eT), C.byref(nf))
    return ns, [tuple(buf[3 * i:3 * i + 3]) for i in range(max(ns, 0))], eT.value, nf.value


def test_conv_frames_and_segments_match_python(tiny, large):
    L = _lib.lib()
    assert int(tiny[0]["n_short"]) == 32037 and tiny[0]["speech"].shape[0] == 328123
    for n in counts(tiny):
        assert L.dawn_hubert_conv_frames(large, n) == py_conv_frames(n), n
        segs, eT, nf = py_plan(n)
        ns, got, geT, gnf = c_plan(large, n)
        assert (ns, got, geT, gnf) == (len(segs), segs, eT, nf), (n, got, segs)
        for s, ln, _ in segs[:-1]:
            assert ln == 320080 or s + ln == n                    # 80 samples of right context, clamped to n
    assert [len(py_plan(n)[0]) for n in counts(tiny)] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2]
    # the golden's two lengths give the golden's row counts
    assert c_plan(large, 328123)[2] == tiny[0]["hidden"].shape[0] and c_plan(large, 328123)[3] == tiny[0]["target_audio"].shape[0]
    assert c_plan(large, 32037)[2] == tiny[0]["hidden_short"].shape[0]
    for n in (9, 399, 400, 401, 404, 405):
        want = py_conv_frames(n) if n >= 10 else 0
        assert L.dawn_hubert_conv_frames(large, n) == max(want, 0), n
    # errors: too few samples, too little room
    ns, _, _, _ = c_plan(large, 399)
    assert ns < 0 and "399" in L.dawn_last_error().decode()
    ns, _, _, _ = c_plan(large, 640000, room=1)
    assert ns < 0 and "room" in L.dawn_last_error().decode()


def test_workspace_bytes_nonzero_and_monotone(tiny, large):
    L = _lib.lib()
    sizes = [int(L.dawn_hubert_workspace_bytes(large, n)) for n in sorted(counts(tiny))]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes), sizes
    assert int(L.dawn_hubert_workspace_bytes(large, 399)) == 0
    # one 20 s segment at hubert-large widths: the qkv rows alone are 12 MB, the first conv's output 128 MB
    assert 128 << 20 < sizes[sorted(counts(tiny)).index(320080)] < 1 << 30


def test_launching_entries_refuse_before_touching_memory(large):
    """Every refusal below is decided on the host before the first launch, so dummy device pointers are never dereferenced."""
    L = _lib.lib()
    p = 0x10000
    assert L.dawn_hubert_features(large, p, 399, None, p, p, 1 << 40, None) != 0 and "399" in L.dawn_last_error().decode()
    assert L.dawn_hubert_features(large, p, 400, None, p, p, 1 << 40, None) != 0 and "25 fps" in L.dawn_last_error().decode()
    need = int(L.dawn_hubert_workspace_bytes(large, 32037))
    assert L.dawn_hubert_features(large, p, 32037, None, p, p, need - 1, None) != 0 and "workspace" in L.dawn_last_error().decode()
    assert L.dawn_hubert_encode(large, p, 32037, p, p, 1000, None) != 0 and "workspace" in L.dawn_last_error().decode()
    assert L.dawn_hubert_encode(large, p, 320081, p, p, 1 << 40, None) != 0 and "segment" in L.dawn_last_error().decode()
    assert L.dawn_hubert_encode(large, p, 399, p, p, 1 << 40, None) != 0
    # the kernel's own refusals: aliasing, group width, LDS budget
    assert L.dawn_hubert_pos_conv(p, 10, 128, 2, 32, p, p, p, None) != 0 and "overlaps" in L.dawn_last_error().decode()
    assert L.dawn_hubert_pos_conv(p, 10, 128, 2, 32, p, p, p + 4 * 128 * 9, None) != 0 and "overlaps" in L.dawn_last_error().decode()
    assert L.dawn_hubert_pos_conv(p, 10, 120, 2, 32, p, p, 2 * p, None) != 0 and "gw % 16" in L.dawn_last_error().decode()
    assert L.dawn_hubert_pos_conv(p, 10, 256, 1, 128, p, p, 2 * p, None) != 0 and "64 KB" in L.dawn_last_error().decode()
