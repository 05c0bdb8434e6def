"""-m gpu: the model bundle on the device (csrc/dawn_bundle.hip) and the program without Python (tools/dawn_generate.cpp), on the tiny
five-stage models of tests/test_hip_clip_inputs.py.

* `dawn_bundle_verify`'s checksum kernel against `bundle.checksum` (the index words the writer computed with it): tensors of 1, 2, 63,
  64, 65, 255, 256, 257, 1023 words, one of 65536 + 1 words (it ends one word into its second work item) and one of 2 * 65536 + 77 (three
  items), at the 256-aligned offsets the writer gives them, region and workspace both exactly the queried size between guard bands.  A bit
  flipped in the first and in the last word and two exchanged words are each reported with the tensor's name.
* Round trip from the fixture's PipelineEvaluator: every table entry's device bytes, every cfg blob, the step table.
* Frames from the bundle's handles `torch.equal` to frames from the fixture's own handles: RGB and yuv420p, cond_scale 1 and 2, through
  dawn_generate_clip_media_rate at 16000 Hz and at 22050 Hz.
* tools/dawn_generate.cpp, built by the test and run once per format as a fresh child process under its own time limit: the .y4m
  payload and the rgb file equal the Python host's bytes.
* Refusals that launch nothing and name their cause."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import wave

import numpy as np
import pytest
import torch

from conftest import ROOT
from guarded import GuardedOps
from test_hip_clip_inputs import BBOX_PIPE, H_PIPE, INIT_BLINK2, INIT_POSE6, N_SAMPLES, SEED, T_PIPE, hip, stages  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ITEM_WORDS = 65536                                    # words per work item (include/dawn_hip.h)
WORD_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, ITEM_WORDS + 1, 2 * ITEM_WORDS + 77)


def _open(path):
    from dawn_pytorch_amd import _lib
    L, b = _lib.lib(), C.c_void_p()
    rc = L.dawn_bundle_open(os.fspath(path).encode(), C.addressof(b))
    assert rc == 0, L.dawn_last_error().decode()
    return L, b


# ---------------------------------------------------------------------------------------------- the checksum kernel
@pytest.fixture(scope="module")
def word_bundle(tmp_path_factory):
    from dawn_pytorch_amd import bundle
    rng = np.random.default_rng(7)
    tensors = {f"t.{n}": rng.integers(0, 1 << 32, n, dtype=np.uint32) for n in WORD_COUNTS}
    tensors["t.255"][:] = 0xFFFFFFFF                  # every partial sum carries
    path = str(tmp_path_factory.mktemp("words") / "words.dawn")
    idx = bundle.write_bundle(path, {"decoder": tensors}, {}, {})
    for e in idx["entries"]:                          # the index words ARE bundle.checksum of the tensor's bytes
        assert (e["s1"], e["s2"]) == bundle.checksum(tensors[e["name"]])
    return dict(path=path, index=idx, tensors=tensors)


def test_checksum_kernel_on_guarded_region_and_workspace(word_bundle):
    L, b = _open(word_bundle["path"])
    try:
        idx = word_bundle["index"]
        nbytes, need = int(L.dawn_bundle_device_bytes(b)), int(L.dawn_bundle_verify_workspace_bytes(b))
        n_items = sum(-(-n // ITEM_WORDS) for n in WORD_COUNTS)
        assert nbytes == idx["device_bytes"] and need == (n_items * 24 + 255) // 256 * 256 + (n_items * 16 + 255) // 256 * 256
        offs = sorted(e["offset"] for e in idx["entries"])
        assert len({o % 1024 for o in offs}) >= 3 and all(o % 256 == 0 for o in offs)          # several 256-aligned offsets of one region
        g = GuardedOps()
        mem = g.guarded_out(1, nbytes, name="region", dtype=torch.uint8).view(-1)
        ws = g.guarded_out(1, need, name="workspace", dtype=torch.uint8).view(-1)
        stream = torch.cuda.current_stream().cuda_stream
        assert L.dawn_bundle_upload(b, mem.data_ptr(), nbytes, stream) == 0, L.dawn_last_error().decode()
        torch.cuda.synchronize()
        raw = np.fromfile(word_bundle["path"], dtype=np.uint8)[idx["payload_offset"]:][:nbytes]
        assert torch.equal(mem.cpu(), torch.from_numpy(raw.copy()))
        snapshot = mem.clone()
        assert L.dawn_bundle_verify(b, mem.data_ptr(), nbytes, ws.data_ptr(), need, stream) == 0, L.dawn_last_error().decode()
        torch.cuda.synchronize()
        for r in g.outs:
            r.check_surroundings("write outside the buffer")
        assert torch.equal(mem, snapshot), "verify wrote into the region"
        # the partial pairs of the workspace, added per tensor, are the index words
        part = ws[(n_items * 24 + 255) // 256 * 256:][:n_items * 16].cpu().numpy().view("<u8").reshape(n_items, 2)
        at = 0
        for e in idx["entries"]:
            k = -(-(e["length"] // 4) // ITEM_WORDS)
            s = part[at:at + k].astype(object).sum(0)
            assert (int(s[0]) % (1 << 64), int(s[1]) % (1 << 64)) == (e["s1"], e["s2"]), e["name"]
            at += k
        # corruption of valid device memory: reported with the right tensor name, then repaired
        words = mem.view(torch.int32)
        by = {e["name"]: e for e in idx["entries"]}
        for name, edit in (("t.257", "first"), ("t.1023", "last"), (f"t.{ITEM_WORDS + 1}", "last"), (f"t.{2 * ITEM_WORDS + 77}", "swap"), ("t.1", "first")):
            e = by[name]
            w0, n = e["offset"] // 4, e["length"] // 4
            if edit == "swap":
                i, j = w0 + 5, w0 + ITEM_WORDS + 9                                              # in two different work items
                assert int(words[i]) != int(words[j])
                words[i], words[j] = words[j].clone(), words[i].clone()
            else:
                words[w0 if edit == "first" else w0 + n - 1] ^= 1 << 7
            rc = L.dawn_bundle_verify(b, mem.data_ptr(), nbytes, ws.data_ptr(), need, stream)
            msg = L.dawn_last_error().decode()
            assert rc != 0 and f"stage 'decoder', tensor '{name}'" in msg, (name, edit, msg)
            mem.copy_(snapshot)
        assert L.dawn_bundle_verify(b, mem.data_ptr(), nbytes, ws.data_ptr(), need, stream) == 0
        for r in g.outs:
            r.check_surroundings("write outside the buffer")
    finally:
        L.dawn_bundle_close(b)


# ---------------------------------------------------------------------------------------------- the pipeline's bundle
@pytest.fixture(scope="module")
def model(stages, tmp_path_factory):
    from dawn_pytorch_amd import bundle, ctx
    path = str(tmp_path_factory.mktemp("model") / "tiny.dawn")
    defaults = dict(H=H_PIPE, max_n_frames=T_PIPE, random_seed=SEED, bbox6=BBOX_PIPE, init_pose6=INIT_POSE6, init_blink2=INIT_BLINK2,
                    mean=(2.0, 0.0, -3.5))
    idx = bundle.bundle_from_pipeline(path, stages["pipe"], {f"ddim.{len(stages['steps'])}": stages["steps"]}, defaults)
    return dict(path=path, index=idx, ev=ctx.BundleEvaluator(path))


def test_round_trip_tables_cfgs_steps_defaults(stages, model):
    from dawn_pytorch_amd import bundle
    be, pipe = model["ev"], stages["pipe"]
    n = 0
    for s, (stage, ev) in enumerate(zip(bundle.STAGES, pipe.ev)):
        table = be.table(s)
        assert set(table) == set(ev.weights), stage
        for name, t in ev.weights.items():
            got = be.tensor(stage, name)
            raw = t.contiguous().reshape(-1).view(torch.uint8)
            assert got.data_ptr() == table[name] and table[name] % 256 == 0
            assert torch.equal(got[:raw.numel()], raw) and not bool(got[raw.numel():].any()), (stage, name)
            n += 1
        assert bytes(be.ev[s].cfg) == bytes(ev.cfg), stage
    assert n == sum(1 for e in model["index"]["entries"] if e["kind"] == 0) and n > 50
    want = [{k: st[k] for k in ("t", "t_next", "recip", "recipm1", "sqrt_alpha_next", "c", "sigma")} for st in stages["steps"]]
    assert be.steps(f"ddim.{len(want)}") == want
    d = be.defaults()
    assert (d.H, d.fea_ch, d.latent_dim, d.max_n_frames, d.sampling_step, d.ancestral, d.up_border) == (H_PIPE, 80, 32, T_PIPE, len(want), 0, 0)
    assert list(d.bbox6) == BBOX_PIPE and d.random_seed == SEED and (d.clip.kind, d.clip.q) == (0, 0.9)
    assert list(d.init_pose6) == [np.float32(v) for v in INIT_POSE6]


def _pcm16(samples):
    ch0 = torch.clamp(torch.round(samples.cpu() * 32768), -32768, 32767).to(torch.int16)
    return torch.stack((ch0, ch0.flip(0)), 1).contiguous()


def _pcm_at(rate, n16):
    n = -(-n16 * rate // 16000)
    t = np.arange(n) / rate
    rng = np.random.default_rng(rate)
    ch0 = 9000 * np.sin(2 * np.pi * 220 * t) + 5000 * np.sin(2 * np.pi * 1700 * t + 1) + 800 * rng.standard_normal(n)
    return torch.from_numpy(np.stack((ch0.astype(np.int16), (np.arange(n) * 7919 % 65536 - 32768).astype(np.int16)), 1)).contiguous()


@pytest.mark.parametrize("fmt,cond_scale,rate", [("rgb", 1.0, 16000), ("rgb", 2.0, 22050), ("yuv420p", 1.0, 22050), ("yuv420p", 2.0, 16000)])
def test_frames_from_the_bundle_equal_frames_from_the_fixture(stages, model, fmt, cond_scale, rate):
    st = stages
    pcm = (_pcm16(st["samples"]) if rate == 16000 else _pcm_at(rate, N_SAMPLES)).cuda()
    image = (st["img"].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    out = []
    for pipe, steps in ((st["pipe"], st["steps"]), (model["ev"], model["ev"].steps(f"ddim.{len(st['steps'])}"))):
        a = pipe.args(None, None, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, steps, cond_scale=cond_scale, seed=SEED, fmt=fmt,
                      mean=(2.0, 0.0, -3.5), chunk=2, H=H_PIPE)
        m = pipe.from_media(a, image=image, pcm=pcm, pcm_rate=rate)
        out.append(pipe.generate_media(m, want_latent=True, want_cond=True))
    torch.cuda.synchronize()
    for k in ("cond", "latent", "frames"):
        assert torch.equal(out[0][k], out[1][k]), k
    assert out[1]["frames"].shape == ((T_PIPE, H_PIPE * H_PIPE * 3 // 2) if fmt == "yuv420p" else (T_PIPE, H_PIPE, H_PIPE, 3))


# ---------------------------------------------------------------------------------------------- the program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tools/dawn_generate.cpp with the host compiler: it has no device code, only the HIP runtime API and the library."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path_factory.mktemp("dawn_generate") / "dawn_generate")
    libdir = os.path.join(ROOT, "dawn-pytorch_amd")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(rocm, "include"),
                        os.path.join(ROOT, "tools", "dawn_generate.cpp"), "-L", libdir, "-ldawn_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                        f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{os.path.join(rocm, 'lib')}", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_program_output_equals_the_python_host(stages, model, program, tmp_path):
    """One WAV (stereo, 22050 Hz) and one PPM written here; the program runs once per format, each a fresh child under its own time limit.
    A child that dies of a signal or runs into the limit ends the test at once: nothing more is started on the GPU."""
    st, be = stages, model["ev"]
    rate = 22050
    pcm = _pcm_at(rate, N_SAMPLES)
    with wave.open(str(tmp_path / "a.wav"), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(rate); f.writeframes(pcm.numpy().astype("<i2").tobytes())
    image = (st["img"].permute(1, 2, 0) * 255).round().to(torch.uint8).contiguous()
    (tmp_path / "f.ppm").write_bytes(b"P6\n%d %d\n255\n" % (H_PIPE, H_PIPE) + image.cpu().numpy().tobytes())
    want = {}
    for fmt in ("yuv420p", "rgb"):                      # the Python host, from the bundle's defaults as the program reads them
        d = be.defaults()
        a = be.args(None, None, list(d.bbox6), list(d.init_pose6), list(d.init_blink2), d.max_n_frames, be.steps(f"ddim.{d.sampling_step}"),
                    init_pose=list(d.init_pose6), init_eye=list(d.init_blink2), cond_scale=d.cond_scale, x0_clip=("dynamic", d.clip.q),
                    seed=d.random_seed, fmt=fmt, mean=tuple(d.mean), chunk=16, H=d.H)
        want[fmt] = be.generate_media(be.from_media(a, image=image, pcm=pcm.cuda(), pcm_rate=rate))["frames"].cpu().numpy().tobytes()
    torch.cuda.synchronize()
    for fmt, ext in (("y4m", "y4m"), ("rgb", "rgb")):
        out = tmp_path / f"clip.{ext}"
        try:
            r = subprocess.run([program, "--bundle", model["path"], "--wav", str(tmp_path / "a.wav"), "--image", str(tmp_path / "f.ppm"),
                                "--out", str(out), "--format", fmt], capture_output=True, text=True, timeout=120)
        except subprocess.TimeoutExpired:
            pytest.exit("dawn_generate ran into its time limit: no further GPU work", returncode=1)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            pytest.exit(f"dawn_generate died with status {r.returncode}: no further GPU work\n{r.stderr[-2000:]}", returncode=1)
        assert r.returncode == 0, r.stderr
        data = out.read_bytes()
        if fmt == "rgb":
            assert data == want["rgb"]
            continue
        head = b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (H_PIPE, H_PIPE)
        frame = H_PIPE * H_PIPE * 3 // 2
        assert data[:len(head)] == head and len(data) == len(head) + T_PIPE * (6 + frame)
        body = data[len(head):]
        assert all(body[t * (6 + frame):][:6] == b"FRAME\n" for t in range(T_PIPE))
        assert b"".join(body[t * (6 + frame) + 6:][:frame] for t in range(T_PIPE)) == want["yuv420p"]
    # a refusal: the library's message and the program's refusal status
    r = subprocess.run([program, "--bundle", str(tmp_path / "f.ppm"), "--wav", str(tmp_path / "a.wav"), "--image", str(tmp_path / "f.ppm"),
                        "--out", str(tmp_path / "x.y4m")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "magic" in r.stderr


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_name_their_cause(stages, model, tmp_path):
    from dawn_pytorch_amd import _lib, bundle, ctx
    L, b = _open(model["path"])
    stream = torch.cuda.current_stream().cuda_stream
    try:
        nbytes, need = int(L.dawn_bundle_device_bytes(b)), int(L.dawn_bundle_verify_workspace_bytes(b))
        g = GuardedOps()
        mem = g.guarded_out(1, nbytes, name="region", dtype=torch.uint8).view(-1)
        ws = g.guarded_out(1, need, name="workspace", dtype=torch.uint8).view(-1)
        assert L.dawn_bundle_upload(b, mem.data_ptr(), nbytes - 1, stream) != 0                  # device memory one byte short
        msg = L.dawn_last_error().decode()
        assert "dawn_bundle_upload" in msg and f"device memory of {nbytes - 1} bytes, {nbytes} needed" in msg
        assert L.dawn_bundle_verify(b, mem.data_ptr(), nbytes - 1, ws.data_ptr(), need, stream) != 0
        assert "dawn_bundle_verify" in L.dawn_last_error().decode() and "dawn_bundle_device_bytes" in L.dawn_last_error().decode()
        assert L.dawn_bundle_verify(b, mem.data_ptr(), nbytes, ws.data_ptr(), need - 1, stream) != 0   # a workspace below the query
        msg = L.dawn_last_error().decode()
        assert f"workspace of {need - 1} bytes, {need} needed (dawn_bundle_verify_workspace_bytes)" in msg
        assert L.dawn_bundle_upload(b, mem.data_ptr() + 16, nbytes, stream) != 0 and "256-byte aligned" in L.dawn_last_error().decode()
        torch.cuda.synchronize()
        for r in g.outs:                                                                        # nothing was written anywhere
            r.check_surroundings("write outside the buffer")
            assert bool((r.payload == 255).all()), r.name
    finally:
        L.dawn_bundle_close(b)
    # a bundle written for another ABI number: refused on the host, by open
    other = tmp_path / "abi7.dawn"
    bundle.bundle_from_pipeline(other, stages["pipe"], {}, dict(H=H_PIPE), abi=7)
    with pytest.raises(_lib.DawnHipError, match="abi: written for ABI 7, this library is ABI 8"):
        ctx.BundleEvaluator(other)
    # a missing stage: named, before any handle is made
    pipe = stages["pipe"]
    tables = {s: ev.weights for s, ev in zip(bundle.STAGES, pipe.ev) if s != "blink"}
    cfgs = {s: ev.cfg for s, ev in zip(bundle.STAGES, pipe.ev) if s != "blink"}
    missing = tmp_path / "noblink.dawn"
    bundle.write_bundle(missing, tables, cfgs, {"defaults": bundle.defaults_struct(H=H_PIPE)})
    with pytest.raises(_lib.DawnHipError, match="dawn_bundle_create_handles.*stage 'blink' is missing"):
        ctx.BundleEvaluator(missing)
