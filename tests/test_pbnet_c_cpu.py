"""No-GPU checks of the windowed PBnet attention and the C-side pose / blink stage (include/dawn_hip.h: dawn_attn_win32, dawn_pbnet_*,
dawn_pose_blink_stage; csrc/dawn_pbnet.hip): the entries are exported and bound, the ctypes mirror of `dawn_pbnet_cfg` has the C layout,
`dawn_pbnet_create` accepts the table ctx.pbnet_named_weights builds and names the entry it misses, the O(window) bias table of
`PoseBlinkGenerator.rel_bias` is the band of the dense (heads, T, T) table, and the workspace is linear in T.  Nothing is launched: the
weight pointers are dummies."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import load_golden
from dawn_pytorch_amd import _lib, ctx
from dawn_pytorch_amd.pbnet import PoseBlinkGenerator
from oracle.ops_ref import RefOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dawn_attn_win32", "dawn_pbnet_create", "dawn_pbnet_destroy", "dawn_pbnet_workspace_bytes", "dawn_pbnet_generate",
       "dawn_pose_blink_workspace_bytes", "dawn_pose_blink_stage")
MODELS = {"pose": "transformerreemb6", "blink": "transformerreemb5"}


def tiny(name):
    g = load_golden("pbnet_tiny.npz")
    sd = {k.split(":", 2)[2]: torch.from_numpy(g[k]) for k in g if k.startswith(f"sd:{name}:")}
    return PoseBlinkGenerator(sd, archiname=MODELS[name], num_heads=int(g["heads"]), device="cpu", ops=RefOps())


def shipped_cfg(in_dim=6, win=100):
    """The decoders UVG configures: audio 1024, latent 256, d 64, 4 heads, ff 1024, 4 layers."""
    cfg = ctx.PbnetCfg()
    cfg.in_dim, cfg.audio_dim, cfg.latent_dim, cfg.d, cfg.heads, cfg.ff, cfg.n_layers = in_dim, 1024, 256, 64, 4, 1024, 4
    cfg.win, cfg.nrot, cfg.eps = win, 2, 1e-5
    return cfg


def names_of(cfg):
    """The weight names include/dawn_hip.h lists for this topology."""
    out = ["firstposeEmbedding.weight", "firstposeEmbedding.bias", "audioEmbedding.weight", "audioEmbedding.bias", "ztimelinear.weight",
           "ztimelinear.bias", "init_proj.bias", "finallayer.weight", "finallayer.bias", "init_temporal_attn.fn.norm.gamma",
           "init_temporal_attn.fn.norm.beta", "init_temporal_attn.fn.fn.to_qkv.weight", "init_temporal_attn.fn.fn.to_out.weight",
           "init_temporal_attn.fn.fn.rotary_emb.freqs", "bias_tgt.rel", "bias_mem.rel", "mem_kv.w"]
    for i in range(cfg.n_layers):
        p = f"seqTransDecoder.decoder_layers.{i}."
        out += [p + f for f in ("self_attn.to_qkv.weight", "self_attn.to_out.weight", "multihead_attn.to_q.weight",
                                "multihead_attn.to_out.weight", "ffn.linear1.weight", "ffn.linear1.bias", "ffn.linear2.weight",
                                "ffn.linear2.bias", "layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias",
                                "layer_norm3.weight", "layer_norm3.bias")]
    return out


def create(cfg, names):
    """dawn_pbnet_create with dummy non-null pointers -> (rc, handle)."""
    L = _lib.lib()
    arr = (ctx.NamedPtr * max(1, len(names)))()
    keep = [n.encode() for n in names]
    for i, n in enumerate(keep):
        arr[i].name, arr[i].ptr = n, 0x1000 + 256 * i
    h = C.c_void_p()
    rc = L.dawn_pbnet_create(C.addressof(cfg), C.addressof(arr), len(names), C.addressof(h))
    return rc, h


@pytest.fixture(scope="module")
def shipped():
    hs = []
    for in_dim, win in ((6, 100), (2, 200)):
        rc, h = create(shipped_cfg(in_dim, win), names_of(shipped_cfg()))
        assert rc == 0 and h.value, _lib.lib().dawn_last_error().decode()
        hs.append(h)
    yield hs
    for h in hs:
        _lib.lib().dawn_pbnet_destroy(h)


def test_entries_exported_bound_and_abi_unchanged():
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", src), f"{n} not declared in include/dawn_hip.h"
        assert hasattr(L, n), f"{n} not exported by libdawn_hip.so"
        assert n in _lib.SIGNATURES, f"{n} not bound in _lib.SIGNATURES"
    assert L.dawn_abi_version() == 8
    assert L.dawn_pbnet_workspace_bytes.restype is C.c_size_t and L.dawn_pose_blink_workspace_bytes.restype is C.c_size_t


def test_cfg_layout_matches_header():
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    body = src[src.index("typedef struct dawn_pbnet_cfg {") + 31:src.index("} dawn_pbnet_cfg;")]
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
    assert [f[0] for f in fields] == [f[0] for f in ctx.PbnetCfg._fields_]
    assert [f[0] for f in fields] == ["in_dim", "audio_dim", "latent_dim", "d", "heads", "ff", "n_layers", "win", "nrot", "eps"]
    assert all(ty in ("int", "float") for _, ty, _ in fields)
    assert C.sizeof(ctx.PbnetCfg) == 4 * sum(n for _, _, n in fields) == 40
    for (name, ty, n), (_, cty) in zip(fields, ctx.PbnetCfg._fields_):
        assert C.sizeof(cty) == 4 * n and (cty is C.c_float) == (ty == "float"), name


@pytest.mark.parametrize("name", list(MODELS))
def test_create_accepts_the_python_table_and_names_what_is_missing(name):
    L = _lib.lib()
    gen = tiny(name)
    cfg, table = ctx.pbnet_cfg(gen), ctx.pbnet_named_weights(gen)
    assert (cfg.in_dim, cfg.audio_dim, cfg.latent_dim, cfg.d, cfg.heads, cfg.ff, cfg.n_layers, cfg.nrot) == \
        ({"pose": 6, "blink": 2}[name], 48, 24, 64, 4, 96, 2, 2)
    assert cfg.win == {"pose": 100, "blink": 200}[name]
    assert set(table) == set(names_of(cfg))                       # the names the Python side builds = the names the header lists
    hd = cfg.heads * 32
    assert tuple(table["mem_kv.w"].shape) == (cfg.n_layers * 2 * hd, cfg.d) and table["mem_kv.w"].is_contiguous()
    for i in range(cfg.n_layers):
        p = f"seqTransDecoder.decoder_layers.{i}.multihead_attn."
        assert torch.equal(table["mem_kv.w"][2 * i * hd:(2 * i + 1) * hd], gen.w[p + "to_k.weight"])
        assert torch.equal(table["mem_kv.w"][(2 * i + 1) * hd:(2 * i + 2) * hd], gen.w[p + "to_v.weight"])
    assert tuple(table["bias_tgt.rel"].shape) == tuple(table["bias_mem.rel"].shape) == (cfg.heads, 2 * cfg.win + 1)
    rc, h = create(cfg, list(table))
    assert rc == 0 and h.value, L.dawn_last_error().decode()
    L.dawn_pbnet_destroy(h)
    for gone in ("seqTransDecoder.decoder_layers.1.ffn.linear2.weight", "mem_kv.w", "bias_mem.rel", "finallayer.bias",
                 "init_temporal_attn.fn.fn.rotary_emb.freqs"):
        rc, h = create(cfg, [n for n in table if n != gone])
        assert rc != 0 and not h.value and f"'{gone}'" in L.dawn_last_error().decode(), (gone, L.dawn_last_error().decode())


def test_create_refuses_unusable_sizes_and_python_refuses_a_wrong_to_qkv():
    L = _lib.lib()
    for edit, word in ((dict(nrot=17), "nrot"), (dict(nrot=-1), "nrot"), (dict(d=0), "d = 0"), (dict(ff=0), "ff = 0"),
                       (dict(audio_dim=0), "audio_dim = 0"), (dict(win=-1), "win = -1")):
        cfg = shipped_cfg()
        for k, v in edit.items():
            setattr(cfg, k, v)
        rc, h = create(cfg, names_of(shipped_cfg()))
        assert rc != 0 and not h.value and word in L.dawn_last_error().decode(), (edit, L.dawn_last_error().decode())
    # only pointers reach dawn_pbnet_create: the height of a to_qkv is refused, by name, where its shape is still known
    for key in ("init_temporal_attn.fn.fn.to_qkv.weight", "seqTransDecoder.decoder_layers.1.self_attn.to_qkv.weight"):
        gen = tiny("pose")
        gen.w[key] = gen.w[key][:-32].contiguous()
        with pytest.raises(_lib.DawnHipError, match=re.escape(f"'{key}'")):
            ctx.pbnet_named_weights(gen)


@pytest.mark.parametrize("name", list(MODELS))
def test_rel_bias_is_the_band_of_the_dense_table(name):
    T = 450
    gen = tiny(name)
    win, heads = gen.window, gen.heads
    dense_t, dense_m, rc, rs = gen._per_length(T)
    rel = torch.arange(T)[None, :] - torch.arange(T)[:, None]
    band = rel.abs() <= win
    assert bool((~band).any())                                     # the window cuts at this length, for both architectures
    expanded = {}
    for which, dense in (("tgt", dense_t), ("mem", dense_m)):
        rb = gen.rel_bias(which)
        assert tuple(rb.shape) == (heads, 2 * win + 1) and rb.dtype == torch.float32 and not rb.is_cuda
        ex = torch.full((heads, T, T), -1e8)
        ex[:, band] = rb[:, (rel + win)[band]]
        assert torch.equal(dense[:, band], ex[:, band])
        assert bool((dense[:, ~band] <= -9e7).all())
        expanded[which] = ex
    ops, hd = RefOps(), heads * 32
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(T, hd, generator=g) for _ in range(3))
    for which, dense in (("tgt", dense_t), ("mem", dense_m)):
        assert torch.equal(ops.attn_bias32(q, k, v, heads, expanded[which], rc, rs, 32 ** -0.5),
                           ops.attn_bias32(q, k, v, heads, dense, rc, rs, 32 ** -0.5))


def test_workspace_bytes_linear_in_T(shipped):
    L = _lib.lib()
    for h in shipped:
        b = [int(L.dawn_pbnet_workspace_bytes(h, T)) for T in (10000, 20000, 30000)]
        assert b[0] > 0 and b[1] - b[0] == b[2] - b[1]
        per_frame = (b[1] - b[0]) / 10000
        assert per_frame == 3528 * 4                               # the buffer list of include/dawn_hip.h at the shipped widths
        for T in (1, 7, 200, 1600, 62000):
            got = int(L.dawn_pbnet_workspace_bytes(h, T))
            assert got == b[0] + (T - 10000) * 3528 * 4 and got <= T * (16 << 10) + (1 << 20)
        assert int(L.dawn_pbnet_workspace_bytes(h, 62000)) < 1 << 30
        assert int(L.dawn_pbnet_workspace_bytes(h, 0)) == 0
    st = [int(L.dawn_pose_blink_workspace_bytes(shipped[0], shipped[1], T)) for T in (10000, 20000, 30000)]
    assert st[1] - st[0] == st[2] - st[1] == 10000 * 3528 * 4
    assert st[0] == 256 + int(L.dawn_pbnet_workspace_bytes(shipped[0], 10000))


def test_launching_entries_refuse_before_touching_memory(shipped):
    """Every refusal below is decided on the host before the first launch, so dummy device pointers are never dereferenced."""
    L = _lib.lib()
    pose, blink = shipped
    p, big = 0x10000, 1 << 40
    err = lambda: L.dawn_last_error().decode()                                              # noqa: E731
    assert L.dawn_pbnet_generate(pose, p, p, 1024, p, 0, 1 << 50, 6, p, big, None) != 0 and "T = 0" in err()
    assert L.dawn_pbnet_generate(pose, p, p, 1024, None, 10, 1 << 50, 6, p, big, None) != 0 and "NULL" in err()
    need = int(L.dawn_pbnet_workspace_bytes(pose, 10))
    assert L.dawn_pbnet_generate(pose, p, p, 1024, p, 10, 1 << 50, 6, p, need - 1, None) != 0 and "workspace" in err()
    assert L.dawn_pbnet_generate(pose, p, p, 1024, p, 10, p + 64, 6, p, need, None) != 0 and "overlaps" in err()
    assert L.dawn_pbnet_generate(pose, p, p, 1023, p, 10, 1 << 50, 6, p, need, None) != 0 and "ld_audio" in err()
    assert L.dawn_pbnet_generate(pose, p, p, 1024, p, 10, 1 << 50, 5, p, need, None) != 0 and "ld_out" in err()
    ip, ib = (C.c_float * 6)(), (C.c_float * 2)()
    sneed = int(L.dawn_pose_blink_workspace_bytes(pose, blink, 10))
    stage = lambda T, zb, ws, out=1 << 50: L.dawn_pose_blink_stage(pose, blink, p, 1024, T, ip, ib, p, zb, out, 6, 1 << 51, 2, p, ws,  # noqa: E731
                                                                   None)
    assert stage(0, p, big) != 0 and "T = 0" in err()
    assert stage(10, None, big) != 0 and "NULL" in err()
    assert stage(10, p, sneed - 1) != 0 and "workspace" in err()
    assert stage(10, p, sneed, out=p + 8) != 0 and "overlaps" in err()
    assert L.dawn_pose_blink_stage(blink, pose, p, 1024, 10, ip, ib, p, p, 1 << 50, 6, 1 << 51, 2, p, sneed, None) != 0 and "in_dim" in err()
    # the kernel's own refusals
    a = lambda Tq, Tk, win, ld=128, nrot=0: L.dawn_attn_win32(p, ld, p, 128, p, 128, Tq, Tk, 4, win, None, None, None, nrot, 1.0, p, 128,  # noqa: E731
                                                              None)
    assert a(10, 10, -1) != 0 and "win < 0" in err()
    assert a(14, 10, 3) != 0 and "without a key" in err()
    assert a(10, 10, 3, ld=127) != 0 and "strides" in err()
    assert a(10, 10, 3, nrot=2) != 0 and "nrot" in err()
