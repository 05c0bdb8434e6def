"""No GPU: the model bundle format (dawn_pytorch_amd/bundle.py, include/dawn_hip.h "model bundle").

* `write_bundle` / `read_index` round trip on synthetic tables: fp32 and 2-byte tensors with odd element counts, names with dots, a
  zero-length tensor refused; offsets 256-aligned, padding bytes zero, checksums equal `bundle.checksum`.
* `bundle.checksum` against a big-integer Python loop.
* The C loader's host entries (open / cfg / host / table sizes) on the same file, and its refusals by name.
* tools/bundle_check.cpp, a stand-alone program over csrc/dawn_bundle_format.h and tools/media_files.h, built with the host compiler and
  -fsanitize=address,undefined and run as its own process: a valid bundle, every truncation of its header and index, every index field
  set to 0 / 2^63 / 2^64 - 1, two overlapping entries, a WAV whose chunk size exceeds the file, a PPM with a short raster.  Every case
  ends with exit status 0 (accepted) or 3 (the program's refusal); a sanitizer report would end it with another status."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from dawn_pytorch_amd import _lib, bundle, ctx

CSRC = os.path.join(ROOT, "dawn-pytorch_amd", "csrc")
ACCEPTED, REFUSED = 0, 3


def big_checksum(raw: bytes):
    raw = raw + b"\0" * (-len(raw) % 4)
    s1 = s2 = 0
    for i in range(len(raw) // 4):
        w = int.from_bytes(raw[4 * i:4 * i + 4], "little")
        s1 += w
        s2 += (i + 1) * w
    return s1 % (1 << 64), s2 % (1 << 64)


def synthetic():
    g = torch.Generator().manual_seed(0)
    tables = {
        "hubert": {"conv.0.w": torch.randn(5, 7, generator=g), "layers.0.ln1.g": torch.randn(1, generator=g)},
        "unet": {"downs.0.rb1.w1s": torch.randn(333, generator=g).to(torch.bfloat16),             # an odd 2-byte count: 2 padding bytes
                 "rel_emb": torch.randn(64, 8, generator=g), "mid.tattn.wqkv_s": torch.randn(3, generator=g).to(torch.float16),
                 "bytes": torch.arange(0, 255, dtype=torch.uint8)},                              # 255 bytes: one padding byte
        "decoder": {"first_w3": np.arange(147 * 4, dtype=np.float32).reshape(147, 4)},
    }
    hub, unet = ctx.HubertCfg(), ctx.UnetCfg()
    hub.n_conv, hub.hidden, hub.eps = 7, 1024, 1e-5
    unet.dim, unet.win = 64, 40
    steps = [dict(t=999 - i, t_next=998 - i, recip=1.5 + i, recipm1=0.5, sqrt_alpha_next=0.25, c=0.125, sigma=float(i)) for i in range(3)]
    host = {"defaults": bundle.defaults_struct(H=32, max_n_frames=5, mean=(2.0, 0.0, -3.5)), "steps.ddim.3": bundle.steps_blob("ddim.3", steps),
            "notes": b"seventeen bytes.."}
    return tables, {"hubert": hub, "unet": unet}, host, steps


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bundle") / "tiny.dawn")
    tables, cfgs, host, steps = synthetic()
    return dict(path=path, index=bundle.write_bundle(path, tables, cfgs, host), tables=tables, cfgs=cfgs, host=host, steps=steps)


def raw_of(t):
    return t.tobytes() if isinstance(t, np.ndarray) else t.contiguous().view(torch.uint8).numpy().tobytes()


def test_checksum_against_big_integers():
    rng = np.random.default_rng(1)
    for n in (0, 1, 3, 4, 5, 255, 1024, 70001):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert bundle.checksum(raw) == big_checksum(raw), n
    big = b"\xff" * (4 * 100000)                                       # s2 wraps: 2^32 * 100000^2 / 2 > 2^64
    assert bundle.checksum(big) == big_checksum(big) and big_checksum(big)[1] != (2 ** 32 - 1) * 100000 * 100001 // 2
    a = np.arange(12, dtype=np.uint32)
    b = a.copy(); b[[2, 9]] = b[[9, 2]]                                # two exchanged unequal words: s1 stays, s2 moves
    assert bundle.checksum(a)[0] == bundle.checksum(b)[0] and bundle.checksum(a)[1] != bundle.checksum(b)[1]
    c = a.copy(); c[11] ^= 1 << 31
    assert bundle.checksum(a)[0] != bundle.checksum(c)[0]


def test_write_and_read_index_round_trip(tiny):
    idx, path = tiny["index"], tiny["path"]
    data = open(path, "rb").read()
    assert idx["version"] == 1 and idx["abi"] == _lib.lib().dawn_abi_version() == 8
    assert idx["file_bytes"] == len(data) and idx["payload_offset"] % 256 == 0 and idx["device_bytes"] % 256 == 0
    assert 64 + idx["index_bytes"] <= idx["payload_offset"]
    want = {(s, n): raw_of(t) for s, tab in tiny["tables"].items() for n, t in tab.items()}
    dev = [e for e in idx["entries"] if e["kind"] == bundle.KIND_DEVICE]
    assert {(e["stage"], e["name"]) for e in dev} == set(want) and len(dev) == 7
    covered = np.zeros(idx["device_bytes"], dtype=bool)
    for e in dev:
        raw = want[(e["stage"], e["name"])]
        assert e["offset"] % 256 == 0 and e["length"] == (len(raw) + 3) // 4 * 4 and e["offset"] + e["length"] <= idx["device_bytes"]
        got = data[idx["payload_offset"] + e["offset"]:][:e["length"]]
        assert got[:len(raw)] == raw and got[len(raw):] == b"\0" * (e["length"] - len(raw))
        assert (e["s1"], e["s2"]) == bundle.checksum(got) == big_checksum(raw)
        assert not covered[e["offset"]:e["offset"] + e["length"]].any()
        covered[e["offset"]:e["offset"] + e["length"]] = True
    payload = np.frombuffer(data, dtype=np.uint8)[idx["payload_offset"]:][:idx["device_bytes"]]
    assert not payload[~covered].any(), "bytes between tensors are zero"
    by = {(e["stage"], e["name"]): e for e in idx["entries"]}
    assert by[("unet", "downs.0.rb1.w1s")]["length"] == 668 and by[("unet", "bytes")]["length"] == 256
    assert by[("unet", "downs.0.rb1.w1s")]["dtype"] == bundle.DTYPES["bfloat16"] and by[("decoder", "first_w3")]["dtype"] == bundle.DTYPES["float32"]
    for key, blob in ((("hubert", "cfg"), bytes(tiny["cfgs"]["hubert"])), (("unet", "cfg"), bytes(tiny["cfgs"]["unet"])),
                      (("host", "defaults"), bytes(tiny["host"]["defaults"])), (("host", "steps.ddim.3"), bytes(tiny["host"]["steps.ddim.3"])),
                      (("host", "notes"), tiny["host"]["notes"])):
        e = by[key]
        assert e["kind"] == bundle.KIND_HOST and e["offset"] % 16 == 0 and e["offset"] >= idx["device_bytes"] and e["length"] == len(blob)
        assert data[idx["payload_offset"] + e["offset"]:][:e["length"]] == blob and (e["s1"], e["s2"]) == bundle.checksum(blob)


def test_writer_refusals(tmp_path):
    tables, cfgs, host, _ = synthetic()
    with pytest.raises(ValueError, match="zero-length"):
        bundle.write_bundle(tmp_path / "z.dawn", {"unet": {"empty": torch.zeros(0)}}, {}, {})
    with pytest.raises(ValueError, match="unknown stage"):
        bundle.write_bundle(tmp_path / "s.dawn", {"vocoder": {"w": torch.zeros(1)}}, {}, {})
    with pytest.raises(ValueError, match="ddim.<S>"):
        bundle.steps_blob("ddim.4", [])
    assert C.sizeof(bundle.Defaults) == 136 and bundle.Defaults.clip.offset == 120 and bundle.Defaults.random_seed.offset == 32


def opened(path):
    L, b = _lib.lib(), C.c_void_p()
    rc = L.dawn_bundle_open(os.fspath(path).encode(), C.addressof(b))
    return rc, b, L.dawn_last_error().decode()


def test_c_loader_host_entries(tiny):
    """dawn_bundle_open / _cfg / _host / the size queries: host code, no GPU call."""
    L = _lib.lib()
    rc, b, msg = opened(tiny["path"])
    assert rc == 0, msg
    try:
        assert L.dawn_bundle_device_bytes(b) == tiny["index"]["device_bytes"]
        assert L.dawn_bundle_verify_workspace_bytes(b) == 256 + 256          # 7 work items: a list and 7 pairs, each rounded up to 256
        unet = ctx.UnetCfg()
        assert L.dawn_bundle_cfg(b, 5, C.addressof(unet), C.sizeof(unet)) == 0 and bytes(unet) == bytes(tiny["cfgs"]["unet"])
        assert L.dawn_bundle_cfg(b, 5, C.addressof(unet), C.sizeof(unet) - 4) != 0 and "out_bytes" in L.dawn_last_error().decode()
        pb = ctx.PbnetCfg()
        assert L.dawn_bundle_cfg(b, 1, C.addressof(pb), C.sizeof(pb)) != 0
        assert "stage 'pose' is missing" in L.dawn_last_error().decode()
        p, n = C.c_void_p(), C.c_size_t()
        assert L.dawn_bundle_host(b, b"steps.ddim.3", C.addressof(p), C.byref(n)) == 0
        assert C.string_at(p.value, n.value) == bytes(tiny["host"]["steps.ddim.3"])
        assert L.dawn_bundle_host(b, b"steps.ddim.4", C.addressof(p), C.byref(n)) != 0 and "steps.ddim.4" in L.dawn_last_error().decode()
        region = C.create_string_buffer(16)                                 # any non-NULL address: the table is base + offset, nothing is read
        t, cnt = C.c_void_p(), C.c_int()
        assert L.dawn_bundle_table(b, 5, C.addressof(region), C.addressof(t), C.byref(cnt)) == 0 and cnt.value == 4
        arr = C.cast(t, C.POINTER(ctx.NamedPtr))
        got = {arr[i].name.decode(): arr[i].ptr - C.addressof(region) for i in range(4)}
        assert got == {e["name"]: e["offset"] for e in tiny["index"]["entries"] if e["stage"] == "unet" and e["kind"] == 0}
    finally:
        L.dawn_bundle_close(b)


def patched(tiny, tmp_path, name, edits, cut=None):
    data = bytearray(open(tiny["path"], "rb").read())
    for at, fmt, v in edits:
        struct.pack_into(fmt, data, at, v)
    path = tmp_path / name
    path.write_bytes(bytes(data[:cut]))
    return path


def entry_at(tiny, stage, name):
    """Byte position of an entry in the file."""
    at = 64
    for e in tiny["index"]["entries"]:
        if (e["stage"], e["name"]) == (stage, name):
            return at
        at += 48 + (len(e["name"].encode()) + 7) // 8 * 8
    raise KeyError(name)


def test_c_loader_refusals_name_the_field_or_the_entry(tiny, tmp_path):
    idx = tiny["index"]
    rel, w1s = entry_at(tiny, "unet", "rel_emb"), entry_at(tiny, "unet", "downs.0.rb1.w1s")
    by = {(e["stage"], e["name"]): e for e in idx["entries"]}
    cases = [
        ("magic", [(0, "<B", ord("X"))], None, "magic"),
        ("version", [(8, "<I", 2)], None, "version"),
        ("abi", [(12, "<I", 7)], None, "abi: written for ABI 7, this library is ABI 8"),
        ("size", [], idx["file_bytes"] - 1, "file_bytes"),
        ("index", [(24, "<Q", idx["file_bytes"])], None, "index_bytes"),
        ("leaves", [(rel + 24, "<Q", idx["device_bytes"])], None, "entry 'unet/rel_emb': leaves the device part"),
        ("align", [(rel + 16, "<Q", by[("unet", "rel_emb")]["offset"] + 16)], None, "entry 'unet/rel_emb': offset"),
        ("overlap", [(w1s + 16, "<Q", by[("unet", "rel_emb")]["offset"])], None, "overlaps"),
        ("overflow", [(rel + 16, "<Q", (1 << 64) - 256)], None, "entry 'unet/rel_emb': offset + length overflows"),
        ("zero", [(rel + 24, "<Q", 0)], None, "entry 'unet/rel_emb': length 0"),
        ("struct", [(entry_at(tiny, "unet", "cfg") + 24, "<Q", C.sizeof(ctx.UnetCfg) - 4)], None, "entry 'unet/cfg': 56 bytes, the struct has 60"),
        ("hostsum", [(entry_at(tiny, "host", "notes") + 32, "<Q", 1)], None, "entry 'host/notes': checksum mismatch"),
    ]
    for name, edits, cut, want in cases:
        rc, b, msg = opened(patched(tiny, tmp_path, name + ".dawn", edits, cut))
        assert rc != 0 and not b.value and want in msg, (name, msg)
    # a name given twice in a stage: two names one letter apart, the letter patched in the index
    twice = tmp_path / "twice.dawn"
    bundle.write_bundle(twice, {"pose": {"w.a": torch.ones(3), "w.b": torch.ones(5)}}, {}, {})
    data = bytearray(twice.read_bytes())
    at = data.index(b"w.b")
    data[at + 2] = ord("a")
    twice.write_bytes(bytes(data))
    rc, _, msg = opened(twice)
    assert rc != 0 and "entry 'pose/w.a': name given twice" in msg, msg
    # name padding that is not zero
    data[at + 2:at + 4] = b"bx"
    twice.write_bytes(bytes(data))
    rc, _, msg = opened(twice)
    assert rc != 0 and "name padding" in msg, msg
    rc, _, msg = opened(tmp_path / "absent.dawn")
    assert rc != 0 and "cannot open" in msg


# ------------------------------------------------------------------------------------------------ the sanitizer program
@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bundle_check") / "bundle_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program itself
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I", CSRC,
                        os.path.join(ROOT, "tools", "bundle_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def run(exe, mode, path, want):
    r = subprocess.run([exe, "--abi", "8", mode, os.fspath(path)], capture_output=True, text=True, timeout=120)    # its own process
    assert r.returncode == want, (mode, os.fspath(path), r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r


def test_sanitized_program_on_bundles(prog, tiny, tmp_path):
    assert "OK 12 entries" in run(prog, "bundle", tiny["path"], ACCEPTED).stdout
    out = run(prog, "mutate", tiny["path"], ACCEPTED).stdout
    head = 64 + tiny["index"]["index_bytes"]
    assert f"TRUNCATIONS {head} accepted 0" in out
    n_fields = 2 + 6 + 8 * 12
    line = [ln for ln in out.splitlines() if ln.startswith("FIELDS")][0].split()
    assert int(line[1]) == n_fields and int(line[3]) == 3 * n_fields
    accepted = [ln for ln in out.splitlines() if ln.startswith("ACCEPTED")]
    # what may change without a refusal on the host: the informational dtype of an entry set to 0, and the checksum words of a DEVICE
    # tensor (dawn_bundle_verify compares those, on the GPU); nothing else
    # (and an entry's stage set to 0: it then belongs to the first stage, which is a valid file unless the name exists there)
    dtype_at = {entry_at(tiny, e["stage"], e["name"]) + k for e in tiny["index"]["entries"] for k in (0, 8)}
    sums_at = {entry_at(tiny, e["stage"], e["name"]) + k for e in tiny["index"]["entries"] if e["kind"] == bundle.KIND_DEVICE for k in (32, 40)}
    for ln in accepted:
        at = int(ln.split()[4])
        assert at in sums_at or (at in dtype_at and ln.endswith("= 0")), ln
    assert len(accepted) >= 3 * len(sums_at)
    assert int(line[5]) + int(line[7]) + len(accepted) == 3 * n_fields and int(line[7]) < n_fields
    by = {(e["stage"], e["name"]): e for e in tiny["index"]["entries"]}
    overlap = patched(tiny, tmp_path, "overlap.dawn", [(entry_at(tiny, "unet", "downs.0.rb1.w1s") + 16, "<Q", by[("unet", "rel_emb")]["offset"])])
    assert "overlaps" in run(prog, "bundle", overlap, REFUSED).stderr
    for cut in (0, 63, 64, head - 1, head, tiny["index"]["file_bytes"] - 1):
        run(prog, "bundle", patched(tiny, tmp_path, f"cut{cut}.dawn", [], cut), REFUSED)


def wav_bytes(n_frames=100, channels=2, rate=44100, data_size=None, extensible=False):
    pcm = (np.arange(n_frames * channels) * 37 % 65536 - 32768).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else 1, channels, rate, rate * channels * 2, channels * 2, 16)
    if extensible:
        fmt += struct.pack("<HHIH", 22, 16, 3, 1) + bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 3) + b"abc\0" + \
        b"data" + struct.pack("<I", len(pcm) if data_size is None else data_size) + pcm
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_sanitized_program_on_media_files(prog, tmp_path):
    def case(name, raw, mode, want):
        p = tmp_path / name
        p.write_bytes(raw)
        return run(prog, mode, p, want)
    assert "OK 100 frames, 2 channels, 44100 Hz" in case("ok.wav", wav_bytes(), "wav", ACCEPTED).stdout
    assert "OK 100 frames" in case("ext.wav", wav_bytes(extensible=True), "wav", ACCEPTED).stdout
    assert "leaves the file" in case("long.wav", wav_bytes(data_size=401), "wav", REFUSED).stderr       # chunk size one byte beyond the file
    assert "leaves the file" in case("huge.wav", wav_bytes(data_size=0xFFFFFFFF), "wav", REFUSED).stderr
    good = wav_bytes()
    for cut in range(0, len(good) - 400 + 8, 3):                                                        # every header cut, and into the data
        case(f"cut{cut}.wav", good[:cut], "wav", REFUSED)
    case("float.wav", good[:20] + struct.pack("<H", 3) + good[22:], "wav", REFUSED)
    ppm = b"P6\n# a comment\n5 3\n255\n" + bytes(range(45))
    assert "OK 5 x 3 x 3" in case("ok.ppm", ppm, "pnm", ACCEPTED).stdout
    assert "OK 5 x 3 x 1" in case("ok.pgm", b"P5 5 3 255 " + bytes(15), "pnm", ACCEPTED).stdout
    assert "raster of 44 bytes, 45 needed" in case("short.ppm", ppm[:-1], "pnm", REFUSED).stderr
    for cut in range(len(ppm) - 45 + 1):
        case(f"cut{cut}.ppm", ppm[:cut], "pnm", REFUSED)
    case("maxval.ppm", b"P6 5 3 65535 " + bytes(90), "pnm", REFUSED)
    case("digits.ppm", b"P6 99999999999999999999 3 255 " + bytes(9), "pnm", REFUSED)
    case("ascii.ppm", b"P3 1 1 255 0 0 0", "pnm", REFUSED)
