"""-m gpu: the resampler to 16 kHz (csrc/audio_resample.hip) and the pipeline from PCM at any rate (dawn_generate_clip_media_rate).

* `dawn_resample16k_pcm16` on every case of tests/resample_cases.py -- the ten rates, inputs shorter than the filter, n_out around one
  workgroup -- against the fp64 oracle under the gate |got - y64| <= 2^-23 |y64| + 2^-40, written into a guarded buffer, the workspace
  exactly `dawn_resample16k_workspace_bytes` between guard bands, bit-identical run to run.
* An impulse at 44.1 and 11.025 kHz: every output is one table entry, the tails included, at the gate's absolute term.
* A PCM source that is 2- but not 4-byte aligned; the fp32 entry `torch.equal` to the PCM entry; rate 16000 `torch.equal` to
  `pcm16_to_samples` / a copy.
* `dawn_generate_clip_media_rate` on the tiny five-stage models of tests/test_hip_clip_inputs.py: at 48 and 44.1 kHz bit-identical to
  `dawn_generate_clip` fed with the op's output, at 16 kHz bit-identical to `dawn_generate_clip_media`.
* `VideoGenerator(audio_via_c=True)` on a 44.1 kHz WAV with an empty PATH (no ffmpeg can run)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import GuardedOps
from resample_cases import ALL_CASES, IMPULSE_AT, assert_gate, case_id, impulse, oracle, pcm_for, reference
from test_hip_clip_inputs import BBOX_PIPE, H_PIPE, INIT_BLINK2, INIT_POSE6, N_SAMPLES, SEED, T_PIPE, hip, stages  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def device_pcm(pcm):
    """(n, channels) int16 on the device; one channel goes up as (n,)."""
    t = torch.from_numpy(pcm.copy()).cuda()                  # (the shared reference arrays are read-only)
    return t if pcm.shape[1] > 1 else t[:, 0].contiguous()


# ---------------------------------------------------------------------------------------------- the op under the gate
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_resample_under_the_gate_guarded_and_deterministic(hip, case):
    """The C entry point, its output between guard bands and poisoned, its workspace exactly dawn_resample16k_workspace_bytes between
    guard bands (the table is bytes of every value, so only its surroundings are checked); then the op, which must give the same bits."""
    from dawn_pytorch_amd import _lib
    L = _lib.lib()
    rate, n_frames, channels = case
    pcm, y64 = reference(case)
    src = device_pcm(pcm)
    need = int(L.dawn_resample16k_workspace_bytes(rate))
    g, gw = GuardedOps(), GuardedOps()
    out = g.guarded_out(1, y64.size, name="out").view(-1)
    ws = gw.guarded_out(1, need, name="workspace", dtype=torch.uint8)
    rc = L.dawn_resample16k_pcm16(src.data_ptr(), n_frames, channels, rate, out.data_ptr(), y64.size, ws.data_ptr(), need,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dawn_last_error().decode()
    torch.cuda.synchronize()
    g.verify()                                               # bands intact, no element left as poison
    gw.outs[0].check_surroundings("write outside the workspace")
    assert_gate(out.cpu().numpy(), y64, f"dawn_resample16k_pcm16 {case_id(case)}")
    g2 = GuardedOps()
    again = g2.guarded_out(1, y64.size, name="out").view(-1)
    assert hip.resample_to_16k(src, rate, out=again) is again
    torch.cuda.synchronize()
    g2.verify()
    assert torch.equal(again, out)
    assert hip.resample_to_16k(src, rate).shape == (y64.size,)


@pytest.mark.parametrize("rate,at", [(44100, IMPULSE_AT), (11025, 523)])
def test_impulse_shows_every_table_entry(hip, rate, at):
    """One 32767 among zeros: each output is one coefficient (the tails of the table included) times 32767 / 32768, and the gate's
    absolute term 2^-40 is what it is held to there."""
    pcm = impulse(3000, at, channels=2)
    pcm[:, 1] = 12345                                        # the other channel must not leak
    y64 = oracle(pcm, rate)
    assert (np.abs(y64) > 0).sum() > 60 and 0 < np.abs(y64[np.abs(y64) > 0]).min() < 1e-5
    g = GuardedOps()
    out = g.guarded_out(1, y64.size, name="out").view(-1)
    hip.resample_to_16k(device_pcm(pcm), rate, out=out)
    torch.cuda.synchronize()
    g.verify()
    got = out.cpu().numpy()
    assert_gate(got, y64, f"impulse at {at}, {rate} Hz")
    assert np.array_equal(got == 0, y64 == 0)                # the same outputs are reached by the impulse, and no others


def test_pcm_source_aligned_to_2_bytes_only_and_the_fp32_entry(hip):
    for case in ((44100, 3000, 2), (48000, 3100, 1), (8000, 700, 1)):
        rate, n, channels = case
        pcm, y64 = reference(case)
        buf = torch.zeros(n * channels + 1, dtype=torch.int16, device="cuda")
        buf[1:] = torch.from_numpy(pcm.copy()).flatten().cuda()
        src = buf[1:].view(n, channels) if channels > 1 else buf[1:]
        assert src.data_ptr() % 4 == 2                       # 2- but not 4-byte aligned
        got = hip.resample_to_16k(src, rate)
        want = hip.resample_to_16k(device_pcm(pcm), rate)
        assert torch.equal(got, want)
        assert_gate(got.cpu().numpy(), y64, f"odd-word source {case_id(case)}")
        x32 = (torch.from_numpy(pcm[:, 0].copy()).float() / 32768).cuda()
        g = GuardedOps()
        assert torch.equal(g.resample_to_16k(x32, rate), want), case
        torch.cuda.synchronize()
        assert [r.name for r in g.outs] == ["resample_to_16k.out", "resample_to_16k.ws"]
        for r in g.outs:
            r.check_surroundings("write outside the buffer")


def test_rate_16000_is_the_conversion_alone(hip):
    pcm = pcm_for(16000, 1025, 2, seed=1)
    src = device_pcm(pcm)
    got = hip.resample_to_16k(src, 16000)
    assert torch.equal(got, hip.pcm16_to_samples(src)) and torch.equal(got.cpu(), torch.from_numpy(pcm[:, 0].copy()).float() / 32768)
    x32 = torch.randn(777, generator=torch.Generator().manual_seed(2)).cuda()
    assert torch.equal(hip.resample_to_16k(x32, 16000), x32)


# ---------------------------------------------------------------------------------------------- dawn_generate_clip_media_rate
def _pcm_at(rate):
    """Stereo PCM at `rate` that yields exactly N_SAMPLES samples at 16 kHz: a few tones and noise in channel 0, a pattern in channel 1."""
    n = -(-N_SAMPLES * rate // 16000)
    assert n * 16000 // rate == N_SAMPLES
    t = np.arange(n) / rate
    rng = np.random.default_rng(rate)
    ch0 = 9000 * np.sin(2 * np.pi * 220 * t) + 5000 * np.sin(2 * np.pi * 1700 * t + 1) + 800 * rng.standard_normal(n)
    ch1 = (np.arange(n) * 7919) % 65536 - 32768
    return torch.from_numpy(np.stack((ch0.astype(np.int16), ch1.astype(np.int16)), 1)).contiguous().cuda()


@pytest.mark.parametrize("rate", [48000, 44100])
def test_generate_clip_media_rate_equals_generate_clip_on_the_resampled_samples(hip, stages, rate):
    from dawn_pytorch_amd import _lib
    st, pipe = stages, stages["pipe"]
    pcm = _pcm_at(rate)
    samples = hip.resample_to_16k(pcm, rate)
    assert samples.shape == (N_SAMPLES,)
    kw = dict(seed=SEED, chunk=2)
    want = pipe.generate(pipe.args(samples, st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw), want_latent=True,
                         want_cond=True)
    a = pipe.args(None, st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw)
    m = pipe.from_media(a, pcm=pcm, pcm_rate=rate)
    got = pipe.generate_media(m, want_latent=True, want_cond=True)
    torch.cuda.synchronize()
    for k in ("cond", "latent", "frames"):
        assert torch.equal(got[k], want[k]), k
    # sizes: dawn_generate_bytes plus the 16 kHz samples and the table, each rounded up to 256 bytes
    a256 = lambda n: (n + 255) // 256 * 256                              # noqa: E731
    plain = pipe.args(samples, st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw)
    fresh = pipe.args(None, st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw)
    table = int(_lib.lib().dawn_resample16k_workspace_bytes(rate))
    assert pipe.media_sizes(pipe.from_media(fresh, pcm=pcm, pcm_rate=rate)) == \
        (pipe.sizes(plain)[0], pipe.sizes(plain)[1] + a256(N_SAMPLES * 4) + a256(table))
    # "T above what the audio yields" is judged on n_out: a third of the frames yields too few
    short = pipe.from_media(fresh, pcm=pcm[:pcm.shape[0] // 3].contiguous(), pcm_rate=rate)
    with pytest.raises(_lib.DawnHipError, match="audio yields"):
        pipe.media_sizes(short)


def test_generate_clip_media_rate_at_16000_is_generate_clip_media(stages):
    from dawn_pytorch_amd import _lib
    st, pipe, L = stages, stages["pipe"], _lib.lib()
    ch0 = torch.clamp(torch.round(st["samples"].cpu() * 32768), -32768, 32767).to(torch.int16)
    pcm = torch.stack((ch0, ch0.flip(0)), 1).contiguous().cuda()
    a = pipe.args(None, st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], seed=SEED, chunk=2)
    m = pipe.from_media(a, pcm=pcm)
    want = pipe.generate_media(m, want_latent=True, want_cond=True)
    torch.cuda.synchronize()
    got = {k: torch.full_like(v, 7) for k, v in want.items()}
    a.frames_out, a.latent_out, a.cond_out = got["frames"].data_ptr(), got["latent"].data_ptr(), got["cond"].data_ptr()
    cb, wb = C.c_size_t(0), C.c_size_t(0)
    assert L.dawn_generate_media_rate_bytes(C.addressof(m), 16000, C.byref(cb), C.byref(wb)) == 0, L.dawn_last_error().decode()
    assert (int(cb.value), int(wb.value)) == pipe.media_sizes(m)
    ws = torch.empty(int(wb.value), dtype=torch.uint8, device="cuda")
    rc = L.dawn_generate_clip_media_rate(C.addressof(m), 16000, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dawn_last_error().decode()
    torch.cuda.synchronize()
    for k in ("cond", "latent", "frames"):
        assert torch.equal(got[k], want[k]), k


# ---------------------------------------------------------------------------------------------- VideoGenerator(audio_via_c=True)
def test_video_generator_audio_via_c_needs_no_ffmpeg(hip, tmp_path, monkeypatch):
    """A stereo 44.1 kHz WAV with PATH emptied, so that no ffmpeg can run: target_audio.npy is hubert.process_audio of the samples that
    HipOps.resample_to_16k makes of the file's frames.  The default path on the same file needs ffmpeg and fails without it."""
    import argparse
    import os
    import sys
    import wave
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.hubert import HubertFeatures
    from dawn_pytorch_amd.video_generator import VideoGenerator
    gh = load_golden("hubert_tiny.npz")
    hub = HubertFeatures({k[3:]: torch.from_numpy(v) for k, v in gh.items() if k.startswith("sd/")}, "cuda:0",
                         num_heads=int(gh["num_heads"]), pos_groups=int(gh["pos_groups"]))
    n = 16538                                                # 0.375 s at 44.1 kHz -> 6000 samples at 16 kHz
    rng = np.random.default_rng(0)
    pcm = np.stack(((np.sin(np.arange(n) * 0.02) * 9000 + rng.standard_normal(n) * 800).astype("<i2"),
                    (rng.standard_normal(n) * 3000).astype("<i2")), 1)
    pcm[:3, 0] = (-32768, 32767, 0)
    wav = tmp_path / "a.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(44100); f.writeframes(pcm.tobytes())
    cache = tmp_path / "cache"
    cfg = {"input_size": 128, "max_n_frames": 200, "random_seed": 1234, "mean": [0.0, 0.0, 0.0], "win_width": 40,
           "sampling_step": 2, "ddim_sampling_eta": 1.0, "cond_scale": 1.0, "model_config": {"is_train": True, "pose_dim": 6}}
    args = argparse.Namespace(audio_path=str(wav), image_path=str(tmp_path / "face.png"), output_path=str(tmp_path / "out"),
                              cache_path=str(cache), resolution=128)
    dec = FlowDecoder(bench_decode.lfg_state_dict(0), "cuda:0")
    mk = lambda **kw: VideoGenerator(args, generator=dec, config=cfg, device="cuda:0", allow_random_weights=True, hubert=hub, **kw)   # noqa: E731
    vg = mk(audio_via_c=True)
    assert vg.audio_via_c is True and mk().audio_via_c is False
    monkeypatch.setenv("PATH", "")
    vg.process_audio()
    feats = np.load(cache / "target_audio.npy")
    samples = hip.resample_to_16k(torch.from_numpy(pcm.astype(np.int16)).cuda(), 44100)
    assert samples.shape == (6000,)
    want = hub.process_audio(samples)
    assert feats.shape == want.shape and feats.shape[0] == int(6000 / 16000 * 25) and np.array_equal(feats, want)
    vg.audio_via_c = False                                   # the default path shells out for this file
    with pytest.raises((FileNotFoundError, OSError)):
        vg.process_audio()
