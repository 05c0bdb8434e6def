"""No GPU: what the C-side motion-encode stage adds around its kernels.

* The numpy restatement of the yuv420p ingest (tests/yuv_cases.py) on hand-computed values and on the clamp corners.
* The bundle's optional stage 7, "motion": writer / index round trip, the C loader's host entries on a file whose only stage it is, a
  cfg blob four bytes short refused by name.  dawn_bundle_create_motion makes GPU handles and is not called here.
* ctx.motion_named_weights / ctx.motion_cfg of the tiny encoder built under the CPU op set.
* The .y4m parser of tools/media_files.h in tools/bundle_check.cpp, built with the host compiler and -fsanitize=address,undefined as
  tests/test_bundle_cpu.py builds it, run as a child process: exit status 0 (accepted) or 3 (refused), no sanitizer report."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import motion_cases as mc
import yuv_cases as yc
from conftest import ROOT
from dawn_pytorch_amd import _lib, bundle, ctx

CSRC = os.path.join(ROOT, "dawn-pytorch_amd", "csrc")
ACCEPTED, REFUSED = 0, 3
NEW = ("dawn_yuv420_to_frames", "dawn_motion_create", "dawn_motion_destroy", "dawn_motion_workspace_bytes", "dawn_motion_encode_clip",
       "dawn_reenact_bytes", "dawn_reenact_clip", "dawn_bundle_create_motion")


# ---------------------------------------------------------------------------------------------- the conversion's restatement
def test_restatement_on_hand_computed_values_and_clamp_corners():
    def rgb(y, u, v):
        return tuple(int(c) for c in yc.yuv_to_rgb(y, u, v))
    assert rgb(16, 128, 128) == (0, 0, 0)                      # 298 * 0 + 128 >> 8 = 0
    assert rgb(235, 128, 128) == (255, 255, 255)               # 298 * 219 + 128 = 65390 >> 8 = 255
    # (0,0,0): C = -16, D = E = -128: R = (-4768 - 52352 + 128) >> 8 = -223 -> 0; G = (-4768 + 12800 + 26624 + 128) >> 8 = 135;
    # B = (-4768 - 66048 + 128) >> 8 = -277 -> 0
    assert rgb(0, 0, 0) == (0, 135, 0)
    # (255,255,255): C = 239, D = E = 127: R = (71222 + 51943 + 128) >> 8 = 481 -> 255; G = (71222 - 12700 - 26416 + 128) >> 8 = 125;
    # B = (71222 + 65532 + 128) >> 8 = 534 -> 255
    assert rgb(255, 255, 255) == (255, 125, 255)
    # (255,0,255): D = -128, E = 127: G = (71222 + 12800 - 26416 + 128) >> 8 = 225; B = (71222 - 66048 + 128) >> 8 = 20
    assert rgb(255, 0, 255) == (255, 225, 20)
    # (0,255,0): D = 127, E = -128: R -> 0; G = (-4768 - 12700 + 26624 + 128) >> 8 = 36; B = (-4768 + 65532 + 128) >> 8 = 237
    assert rgb(0, 255, 0) == (0, 36, 237)
    # an arithmetic shift floors: (81,90,240), C = 65, D = -38, E = 112 -> R = (19370 + 45808 + 128) >> 8 = 255; G = (19370 + 3800 - 23296
    # + 128) >> 8 = 2 >> 8 = 0; B = (19370 - 19608 + 128) >> 8 = -110 >> 8 = -1 -> 0 (a shift that truncated toward zero would give 0 too,
    # but (17,128,128): (298 + 128) >> 8 = 1, and (15,128,128): (-298 + 128) >> 8 = -1 -> 0)
    assert rgb(81, 90, 240) == (255, 0, 0) and rgb(17, 128, 128) == (1, 1, 1) and rgb(15, 128, 128) == (0, 0, 0)
    assert (-1 >> 8) == -1 and int(np.int64(-1) >> 8) == -1
    # chroma is replicated over its 2x2 block
    f = np.zeros((1, 12), dtype=np.uint8)
    f[0] = [16, 235, 81, 145, 16, 235, 81, 145, 128, 90, 128, 240]
    out = yc.frames_to_rgb(f, 2, 4)
    assert out.shape == (1, 2, 4, 3) and np.array_equal(out[0, 0], out[0, 1])
    assert tuple(out[0, 0, 0]) == (0, 0, 0) and tuple(out[0, 0, 1]) == (255, 255, 255) and tuple(out[0, 0, 2]) == rgb(81, 90, 240)
    assert tuple(out[0, 1, 3]) == rgb(145, 90, 240)


def test_exhaustive_frame_holds_every_triple_once():
    f = yc.exhaustive_frame()
    assert f.shape == (1, 4096 * 4096 * 3 // 2)
    y, u, v = yc.planes(f, 4096, 4096)
    key = (y[0].astype(np.int64) << 16) | (u[0].repeat(2, 0).repeat(2, 1).astype(np.int64) << 8) | v[0].repeat(2, 0).repeat(2, 1)
    assert np.array_equal(np.sort(key.reshape(-1)), np.arange(1 << 24))


def test_symbols_and_signatures():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n) and n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8 and L.dawn_motion_workspace_bytes.restype is C.c_size_t
    assert C.sizeof(ctx.MotionCfg) == 192 and ctx.MotionCfg.temperature.offset == 8 and ctx.MotionCfg.rp_down.offset == 28 and C.sizeof(ctx.ReenactArgs) == 120
    # host-side refusals of the converter: nothing is launched for them, so no GPU is needed
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    for args, name in (((p, 12, 1, 3, 4, p), "H = 3"), ((p, 18, 1, 2, 6, p), "W = 6"), ((None, 12, 1, 2, 4, p), "in is NULL"),
                       ((p, 12, 1, 2, 4, None), "out is NULL"), ((p, 11, 1, 2, 4, p), "frame_stride = 11"), ((p, 12, 0, 2, 4, p), "T = 0")):
        assert L.dawn_yuv420_to_frames(*args, None) != 0 and name in L.dawn_last_error().decode(), name


# ---------------------------------------------------------------------------------------------- the bundle's motion stage
def synthetic_motion():
    g = torch.Generator().manual_seed(3)
    cfg = ctx.MotionCfg()
    cfg.R, cfg.s, cfg.temperature, cfg.rp_blocks, cfg.bg_blocks, cfg.pf_blocks = 10, 4, 0.1, 2, 1, 3
    cfg.rp_down[0], cfg.rp_down[1], cfg.pf_up[2] = 16, 32, 44
    table = {"rp.down.0.w": torch.randn(27, 16, generator=g), "rp.down.0.ws": torch.randn(333, generator=g).to(torch.bfloat16), "fc.b": torch.randn(6, generator=g)}
    return table, cfg


def opened(path):
    L, b = _lib.lib(), C.c_void_p()
    rc = L.dawn_bundle_open(os.fspath(path).encode(), C.addressof(b))
    return rc, b, L.dawn_last_error().decode()


def test_bundle_motion_stage_round_trip_and_loader(tmp_path):
    assert bundle.STAGES[7] == "motion" and bundle.STAGES[6] == "host" and len(bundle.STAGES) == 8
    table, cfg = synthetic_motion()
    path = tmp_path / "motion.dawn"
    idx = bundle.write_bundle(path, {"motion": table}, {"motion": cfg}, {})
    assert idx == bundle.read_index(path) and idx["version"] == 1
    by = {(e["stage"], e["kind"], e["name"]): e for e in idx["entries"]}
    assert set(by) == {("motion", 0, n) for n in table} | {("motion", 1, "cfg")}
    data = path.read_bytes()
    for n, t in table.items():
        e = by[("motion", 0, n)]
        raw = t.contiguous().view(torch.uint8).numpy().tobytes()
        assert e["offset"] % 256 == 0 and data[idx["payload_offset"] + e["offset"]:][:len(raw)] == raw and (e["s1"], e["s2"]) == bundle.checksum(raw)
    e = by[("motion", 1, "cfg")]
    assert e["length"] == C.sizeof(ctx.MotionCfg) and data[idx["payload_offset"] + e["offset"]:][:e["length"]] == bytes(cfg)
    with pytest.raises(ValueError, match="unknown stage"):                                  # the writer still knows its stages by name
        bundle.write_bundle(tmp_path / "s.dawn", {"vocoder": {"w": torch.zeros(1)}}, {}, {})
    with pytest.raises(ValueError, match="unknown stage"):
        bundle.write_bundle(tmp_path / "h.dawn", {"host": {"w": torch.zeros(1)}}, {}, {})
    # the C loader: a file whose only stage is `motion`
    L = _lib.lib()
    rc, b, msg = opened(path)
    assert rc == 0, msg
    try:
        got = ctx.MotionCfg()
        assert L.dawn_bundle_cfg(b, 7, C.addressof(got), C.sizeof(got)) == 0 and bytes(got) == bytes(cfg)
        assert L.dawn_bundle_cfg(b, 7, C.addressof(got), C.sizeof(got) - 4) != 0 and "out_bytes" in L.dawn_last_error().decode()
        assert L.dawn_bundle_cfg(b, 6, C.addressof(got), C.sizeof(got)) != 0 and "stage 6" in L.dawn_last_error().decode()
        assert L.dawn_bundle_cfg(b, 8, C.addressof(got), C.sizeof(got)) != 0 and "stage 8" in L.dawn_last_error().decode()
        unet = ctx.UnetCfg()
        assert L.dawn_bundle_cfg(b, 5, C.addressof(unet), C.sizeof(unet)) != 0 and "stage 'unet' is missing" in L.dawn_last_error().decode()
        region = C.create_string_buffer(16)
        t, cnt = C.c_void_p(), C.c_int()
        assert L.dawn_bundle_table(b, 7, C.addressof(region), C.addressof(t), C.byref(cnt)) == 0 and cnt.value == 3
        arr = C.cast(t, C.POINTER(ctx.NamedPtr))
        assert {arr[i].name.decode(): arr[i].ptr - C.addressof(region) for i in range(3)} == {n: by[("motion", 0, n)]["offset"] for n in table}
    finally:
        L.dawn_bundle_close(b)
    # a cfg blob four bytes short: refused at open, by name, as unet/cfg is
    at = 64
    for en in idx["entries"]:
        if (en["stage"], en["name"]) == ("motion", "cfg"):
            break
        at += 48 + (len(en["name"].encode()) + 7) // 8 * 8
    raw = bytearray(data)
    struct.pack_into("<Q", raw, at + 24, C.sizeof(ctx.MotionCfg) - 4)
    short = tmp_path / "short.dawn"
    short.write_bytes(bytes(raw))
    rc, b, msg = opened(short)
    assert rc != 0 and not b.value and f"entry 'motion/cfg': {C.sizeof(ctx.MotionCfg) - 4} bytes, the struct has {C.sizeof(ctx.MotionCfg)}" in msg, msg
    # a stage number past the last one is still refused
    struct.pack_into("<I", raw, at, 8)
    short.write_bytes(bytes(raw))
    rc, _, msg = opened(short)
    assert rc != 0 and "stage 8" in msg, msg


# ---------------------------------------------------------------------------------------------- the tiny encoder's table and cfg
def test_named_weights_and_cfg_of_the_tiny_encoder():
    from dawn_pytorch_amd.motion_encoder import MotionEncoder, _Conv
    sds = mc.state_dicts()
    me = MotionEncoder.from_state_dicts(sds["generator"], sds["region_predictor"], sds["bg_predictor"], "cpu", ops=mc.MotionRefOps())
    table = ctx.motion_named_weights(me)
    again = ctx.motion_named_weights(me)
    assert list(table) == list(again) and all(table[k] is again[k] for k in table)        # stable names, the packed images themselves
    # every _Conv the encoder launches, and every tensor of it, appears exactly once
    convs = [*me.rp_hg.enc.downs, *me.rp_hg.ups, me.rp_regions, me.bg_src0, me.bg_drv0, *me.bg_enc.downs[1:], *me.pf_hg.enc.downs, *me.pf_hg.ups,
             me.pf_out]
    assert all(isinstance(c, _Conv) for c in convs)
    want = [t for c in convs for t in (c.w, c.ws, c.bias, c.a, c.b) if t is not None] + [me.fc_w, me.fc_b]
    ids = [id(t) for t in table.values()]
    assert len(set(ids)) == len(ids) and set(ids) == {id(t) for t in want}
    assert id(me.bg_enc.downs[0].w) not in ids                                              # the unsplit first conv is launched by nobody
    nb = mc.TINY["num_blocks"]
    names = {f"{p}.{d}.{i}.{k}" for p in ("rp", "pf") for d, ks in (("down", "w ws bias a b"), ("up", "w bias a b")) for i in range(nb) for k in ks.split()}
    names |= {"rp.regions.w", "rp.regions.bias", "pf.out.w", "pf.out.bias", "bg.src0.w", "bg.src0.ws", "bg.src0.bias", "bg.drv0.w", "bg.drv0.ws",
              "bg.down.0.a", "bg.down.0.b", "fc.w", "fc.b"}
    names |= {f"bg.down.{i}.{k}" for i in range(1, len(me.bg_enc.downs)) for k in "w ws bias a b".split()}
    assert set(table) == names
    cfg = ctx.motion_cfg(me)
    assert (cfg.R, cfg.s, cfg.rp_blocks, cfg.pf_blocks, cfg.bg_blocks) == (mc.R, mc.S, nb, nb, len(me.bg_enc.downs)) and cfg.temperature == mc.TEMPERATURE
    pf = "pixelwise_flow_predictor.hourglass"
    for arr, sd, stem, n in ((cfg.rp_down, sds["region_predictor"], "predictor.encoder.down_blocks", nb),
                             (cfg.rp_up, sds["region_predictor"], "predictor.decoder.up_blocks", nb),
                             (cfg.bg_down, sds["bg_predictor"], "encoder.down_blocks", cfg.bg_blocks),
                             (cfg.pf_down, sds["generator"], pf + ".encoder.down_blocks", nb), (cfg.pf_up, sds["generator"], pf + ".decoder.up_blocks", nb)):
        assert [arr[i] for i in range(ctx.MOTION_MAX_BLOCKS)] == [sd[f"{stem}.{i}.conv.weight"].shape[0] for i in range(n)] + [0] * (ctx.MOTION_MAX_BLOCKS - n)


# ---------------------------------------------------------------------------------------------- the .y4m parser under the sanitizers
@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bundle_check_y4m") / "bundle_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program itself
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                        os.path.join(ROOT, "tools", "bundle_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_y4m_parser_under_the_sanitizers(prog, tmp_path):
    def case(name, raw, want):
        p = tmp_path / name
        p.write_bytes(raw)
        r = subprocess.run([prog, "y4m", os.fspath(p)], capture_output=True, text=True, timeout=120)      # its own process
        assert r.returncode == want, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        return r
    H, W = 4, 8
    fr = yc.random_frames(2, H, W, seed=5)
    ok = "OK 2 frames of 8 x 4, 96 bytes"
    assert ok in case("ok.y4m", yc.y4m_bytes(fr, H, W), ACCEPTED).stdout
    assert ok in case("noc.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H4 F30000:1001 I? A0:0"), ACCEPTED).stdout
    assert ok in case("params.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 H4 W8 C420mpeg2 XYSCSS=420MPEG2", frame_header=b"FRAME Ip XQ=1\n"), ACCEPTED).stdout
    for c in (b"C420", b"C420paldv"):
        assert ok in case(c.decode() + ".y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H4 " + c), ACCEPTED).stdout
    assert "colourspace 'C444'" in case("c444.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H4 C444"), REFUSED).stderr
    assert "colourspace 'C420p10'" in case("p10.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H4 C420p10"), REFUSED).stderr
    assert "interlacing 'It'" in case("it.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H4 It"), REFUSED).stderr
    assert "W6" in case("w6.y4m", yc.y4m_bytes(yc.random_frames(2, 4, 6), 4, 6), REFUSED).stderr
    assert "H3" in case("h3.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8 H3"), REFUSED).stderr
    good = yc.y4m_bytes(fr, H, W)
    assert "frame 1 is cut: 47 bytes, 48 needed" in case("cut.y4m", good[:-1], REFUSED).stderr
    long_head = b"YUV4MPEG2 W8 H4 X" + b"a" * 300
    assert "longer than 256 bytes" in case("long.y4m", yc.y4m_bytes(fr, H, W, header=long_head), REFUSED).stderr
    assert "longer than 256 bytes" in case("longframe.y4m", yc.y4m_bytes(fr, H, W, frame_header=b"FRAME X" + b"b" * 300 + b"\n"), REFUSED).stderr
    assert "no frame" in case("empty.y4m", b"YUV4MPEG2 W8 H4\n", REFUSED).stderr
    assert "not a YUV4MPEG2" in case("not.y4m", b"P6 1 1 255 abc", REFUSED).stderr
    assert "lacks W or H" in case("noh.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W8"), REFUSED).stderr
    assert "bad header token" in case("digits.y4m", yc.y4m_bytes(fr, H, W, header=b"YUV4MPEG2 W99999999999999999999 H4"), REFUSED).stderr
    head = len(good) - 2 * (6 + 48)
    for cut in range(0, head + 6 + 48 + 6 + 2):                                             # every cut of the headers and of the first frame
        case(f"cut{cut}.y4m", good[:cut], REFUSED if cut != head + 6 + 48 else ACCEPTED)
