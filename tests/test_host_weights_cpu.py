"""No-GPU checks of the weight table the C stage hosts share (csrc/dawn_host.h: DawnWeights), through the three creators that only
record pointers (dawn_ctx_create copies from the device inside create, so it cannot run here): with several required names missing
each host reports its own code and the name its create looks up FIRST, leaves *out NULL, and skips table entries without a name.
Nothing is launched: the weight pointers are dummies."""
import ctypes as C

import pytest

from dawn_pytorch_amd import _lib, ctx


def decoder():
    names = ["first_w3", "first_bias", "first.a", "first.b", "final_w7", "final_bias"]
    for i in range(2):
        names += [f"{p}.{i}.{f}" for p in ("downs", "ups") for f in ("w", "bias", "a", "b")]
    names += [f"bott.0.{f}" for f in ("a1", "b1", "a2", "b2", "c1.w", "c1.bias", "c2.w", "c2.bias")]
    return ctx.DecoderCfg(2, 1, (C.c_int * 8)(64, 128, 256)), names


def hubert():
    cfg = ctx.HubertCfg()
    cfg.n_conv = 2
    for i, (k, s) in enumerate(((10, 5), (3, 2))):
        cfg.conv_k[i], cfg.conv_stride[i] = k, s
    cfg.conv_dim, cfg.hidden, cfg.heads, cfg.intermediate, cfg.n_layers = 32, 128, 2, 64, 2
    cfg.pos_k, cfg.pos_groups, cfg.eps = 16, 2, 1e-5
    names = [f"conv.{i}.{f}" for i in range(2) for f in ("w", "b", "g", "be")]
    names += ["fp.g", "fp.b", "fp.w", "fp.bias", "pos.w", "pos.b", "enc_ln.g", "enc_ln.b"]
    names += [f"layers.{i}.{f}" for i in range(2)
              for f in ("ln1.g", "ln1.b", "wqkv", "bqkv", "wo", "bo", "ln2.g", "ln2.b", "w1", "b1", "w2", "b2")]
    return cfg, names


def pbnet():
    cfg = ctx.PbnetCfg()
    cfg.in_dim, cfg.audio_dim, cfg.latent_dim, cfg.d, cfg.heads, cfg.ff, cfg.n_layers = 6, 48, 24, 64, 4, 96, 2
    cfg.win, cfg.nrot, cfg.eps = 100, 2, 1e-5
    names = ["finallayer.weight", "finallayer.bias", "firstposeEmbedding.weight", "firstposeEmbedding.bias", "audioEmbedding.weight",
             "audioEmbedding.bias", "ztimelinear.weight", "ztimelinear.bias", "init_proj.bias", "init_temporal_attn.fn.norm.gamma",
             "init_temporal_attn.fn.norm.beta", "init_temporal_attn.fn.fn.to_qkv.weight", "init_temporal_attn.fn.fn.to_out.weight",
             "init_temporal_attn.fn.fn.rotary_emb.freqs", "bias_tgt.rel", "bias_mem.rel", "mem_kv.w"]
    for i in range(2):
        p = f"seqTransDecoder.decoder_layers.{i}."
        names += [p + f for f in ("self_attn.to_qkv.weight", "self_attn.to_out.weight", "multihead_attn.to_q.weight",
                                  "multihead_attn.to_out.weight", "ffn.linear1.weight", "ffn.linear1.bias", "ffn.linear2.weight",
                                  "ffn.linear2.bias", "layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias",
                                  "layer_norm3.weight", "layer_norm3.bias")]
    return cfg, names


# host: (cfg and full table, its code, its wording, two required names to remove, the one of them its create looks up first).  The
# tests hand the table over in REVERSE, so the expected name is the later one in table order.
HOSTS = {
    "decoder": (decoder, -230, "missing packed weight", ("first.b", "downs.1.bias"), "first.b"),
    "hubert": (hubert, -250, "missing packed weight", ("conv.1.g", "layers.0.wo"), "conv.1.g"),
    "pbnet": (pbnet, -260, "missing weight", ("finallayer.bias", "audioEmbedding.bias"), "audioEmbedding.bias"),
}


def create(host, cfg, names):
    """dawn_<host>_create on dummy non-null pointers; a name of None becomes an entry without a name -> (rc, handle)."""
    arr = (ctx.NamedPtr * len(names))()
    keep = [None if n is None else n.encode() for n in names]
    for i, n in enumerate(keep):
        arr[i].name, arr[i].ptr = n, 0x1000 + 256 * i
    h = C.c_void_p()
    rc = getattr(_lib.lib(), f"dawn_{host}_create")(C.addressof(cfg), C.addressof(arr), len(names), C.addressof(h))
    return rc, h


@pytest.mark.parametrize("host", list(HOSTS))
def test_several_missing_names_report_the_first_looked_up(host):
    L = _lib.lib()
    make, code, wording, gone, first = HOSTS[host]
    cfg, names = make()
    assert set(gone) <= set(names) and first in gone
    rc, h = create(host, cfg, [n for n in reversed(names) if n not in gone])
    msg = L.dawn_last_error().decode()
    assert rc == code and h.value is None, (rc, h.value)
    assert msg == f"dawn_{host}_create: {wording} '{first}'", msg
    # one missing name: the same code, that name
    rc, h = create(host, cfg, [n for n in names if n != gone[0]])
    assert rc == code and h.value is None and L.dawn_last_error().decode() == f"dawn_{host}_create: {wording} '{gone[0]}'"


@pytest.mark.parametrize("host", list(HOSTS))
def test_entries_without_a_name_are_skipped(host):
    L = _lib.lib()
    make, code, _, gone, _ = HOSTS[host]
    cfg, names = make()
    rc, h = create(host, cfg, [None] + names[:5] + [None] + names[5:] + [None])
    assert rc == 0 and h.value, L.dawn_last_error().decode()
    getattr(L, f"dawn_{host}_destroy")(h)
    # ... and a nameless entry does not stand in for a missing one
    rc, h = create(host, cfg, [None if n == gone[0] else n for n in names])
    assert rc == code and h.value is None and f"'{gone[0]}'" in L.dawn_last_error().decode()
