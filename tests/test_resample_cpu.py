"""No-GPU checks of the resampler to 16 kHz (csrc/audio_resample.hip; dawn_generate_clip_media_rate in csrc/dawn_inputs.hip): symbols and
signatures, the two host helpers against the Python formulas, every refusal (refusals come before any launch, so they run without a
device), the oracle of tests/resample_cases.py against its own 80-bit evaluation, dawn_pytorch_amd/audio.py against the oracle under the
gate, the WAV reader, the filter's pass band and stop band on the oracle, and that the gate rejects four defects."""
import ctypes as C
import wave

import numpy as np
import pytest

from dawn_pytorch_amd import _lib, audio, ctx
from resample_cases import (ALL_CASES, IMPULSE_AT, RATES, assert_gate, impulse, case_id, gate_excess, oracle, out_len, pcm_for, plan, reference, table_bytes)

NEW = ("dawn_resample16k_len", "dawn_resample16k_workspace_bytes", "dawn_resample16k_pcm16", "dawn_resample16k_f32",
       "dawn_generate_media_rate_bytes", "dawn_generate_clip_media_rate")
# non-NULL "device pointers", far apart: every call below is refused before anything would read them
SRC, OUT, WS, PCM = 0x10000000, 0x40000000, 0x70000000, 0x90000000


def err():
    return _lib.lib().dawn_last_error().decode()


# ---------------------------------------------------------------------------------------------- symbols, signatures, helpers
def test_symbols_signatures_and_abi():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8
    assert L.dawn_resample16k_len.restype is C.c_long and L.dawn_resample16k_workspace_bytes.restype is C.c_size_t


def test_length_and_workspace_helpers_equal_the_formulas():
    L = _lib.lib()
    for rate in RATES + [1000, 384000, 383999, 16001, 24000]:
        assert int(L.dawn_resample16k_workspace_bytes(rate)) == table_bytes(rate) > 0, rate
        assert table_bytes(rate) % 256 == 0
        for n in (1, 2, 3, 255, 256, 4096, 441000, 10 ** 9 + 7):
            assert int(L.dawn_resample16k_len(n, rate)) == out_len(n, rate) == audio.resample_len(n, rate), (n, rate)
    for rate, n_frames, _ in ALL_CASES:
        assert int(L.dawn_resample16k_len(n_frames, rate)) == n_frames * 16000 // rate
    assert int(L.dawn_resample16k_len(5, 16000)) == 5 and int(L.dawn_resample16k_workspace_bytes(16000)) == 0
    for bad in (999, 384001, 0, -16000):
        assert int(L.dawn_resample16k_len(48000, bad)) == 0 and int(L.dawn_resample16k_workspace_bytes(bad)) == 0, bad
    assert int(L.dawn_resample16k_len(0, 48000)) == 0 and int(L.dawn_resample16k_len(-3, 48000)) == 0
    assert int(L.dawn_resample16k_len(2, 48000)) == 0                 # two frames at 48 kHz are no 16 kHz sample
    # the filter lengths the definition implies: 769 taps at 192 kHz, 193 at 48 kHz, 65 below 16 kHz, one table row where 16000 | rate
    assert [2 * plan(r)[4] + 1 for r in (192000, 48000, 44100, 8000)] == [769, 193, 179, 65]
    assert [plan(r)[0] for r in (192000, 48000, 32000, 44100, 8000, 44101)] == [1, 1, 1, 160, 2, 16000]


# ---------------------------------------------------------------------------------------------- refusals
def test_resample_pcm16_refusals():
    L = _lib.lib()
    need = int(L.dawn_resample16k_workspace_bytes(48000))

    def call(pcm=PCM, n=4800, ch=2, rate=48000, out=OUT, n_out=1600, ws=WS, ws_bytes=need):
        return L.dawn_resample16k_pcm16(pcm, n, ch, rate, out, n_out, ws, ws_bytes, None)
    for k in ("pcm", "out", "ws"):
        assert call(**{k: None}) != 0 and "NULL" in err() and "dawn_resample16k_pcm16" in err(), k
    assert call(pcm=PCM + 1) != 0 and "pcm is not 2-byte aligned" in err()
    assert call(out=OUT + 2) != 0 and "out is not 4-byte aligned" in err()
    assert call(ws=WS + 4) != 0 and "workspace is not 8-byte aligned" in err()
    for ch in (0, 9, -1):
        assert call(ch=ch) != 0 and f"channels = {ch}" in err(), ch
    for rate in (999, 384001, 0, -48000):
        assert call(rate=rate) != 0 and f"rate = {rate}" in err() and "1000 .. 384000" in err(), rate
    for n_out in (1599, 1601, 0, -1):
        assert call(n_out=n_out) != 0 and f"n_out = {n_out}" in err() and "= 1600" in err() and "dawn_resample16k_len" in err(), n_out
    assert call(ws_bytes=need - 1) != 0
    assert "workspace" in err() and str(need - 1) in err() and str(need) in err() and "dawn_resample16k_workspace_bytes" in err()
    assert call(out=WS + 64) != 0 and "out overlaps the workspace" in err()
    assert call(out=WS - 6400 + 4) != 0 and "out overlaps the workspace" in err()       # its last float is the workspace's first bytes
    for n in (0, -5):
        assert call(n=n, n_out=0) != 0 and f"n_frames = {n}" in err(), n
    assert call(n=2, n_out=0) != 0 and "n_out = 0" in err() and "n_frames = 2" in err()
    # 16 kHz: no table, so no workspace is asked for -- the remaining refusals are dawn_pcm16_to_samples' own
    assert call(rate=16000, n_out=1600, ws=None, ws_bytes=0) != 0 and "n_out = 1600" in err() and "= 4800" in err()


def test_resample_f32_refusals():
    L = _lib.lib()
    need = int(L.dawn_resample16k_workspace_bytes(44100))

    def call(x=SRC, n=4410, rate=44100, out=OUT, n_out=1600, ws=WS, ws_bytes=need):
        return L.dawn_resample16k_f32(x, n, rate, out, n_out, ws, ws_bytes, None)
    for k in ("x", "out", "ws"):
        assert call(**{k: None}) != 0 and "NULL" in err() and "dawn_resample16k_f32" in err(), k
    assert call(x=SRC + 2) != 0 and "x is not 4-byte aligned" in err()
    assert call(out=OUT + 1) != 0 and "out is not 4-byte aligned" in err()
    for rate in (999, 384001):
        assert call(rate=rate) != 0 and f"rate = {rate}" in err(), rate
    assert call(n_out=1601) != 0 and "n_out = 1601" in err() and "= 1600" in err()
    assert call(ws_bytes=need - 256) != 0 and str(need - 256) in err() and str(need) in err() and "dawn_resample16k_workspace_bytes" in err()
    assert call(out=WS + need - 4) != 0 and "out overlaps the workspace" in err()
    assert call(n=0, n_out=0) != 0 and "n_frames = 0" in err()
    assert call(n=2, n_out=0) != 0 and "n_out = 0" in err()


def test_generate_clip_media_rate_refusals_without_handles():
    L = _lib.lib()
    cb, wb = C.c_size_t(7), C.c_size_t(7)
    who = "dawn_generate_clip_media_rate"
    assert L.dawn_generate_media_rate_bytes(None, 48000, C.byref(cb), C.byref(wb)) != 0 and "NULL" in err()
    m = ctx.MediaArgs()
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0 and "NULL" in err() and "gen" in err()
    a = ctx.GenerateArgs()
    m.gen = C.pointer(a)
    a.samples, a.img3 = PCM, SRC
    # fp32 samples are 16 kHz samples: a rate needs PCM
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0
    assert who in err() and "pcm is NULL" in err() and "pcm_rate = 48000" in err()
    assert L.dawn_generate_media_rate_bytes(C.addressof(m), 44100, C.byref(cb), C.byref(wb)) != 0
    assert "dawn_generate_media_rate_bytes" in err() and "pcm_rate = 44100" in err()
    m.pcm, m.n_frames, m.channels = PCM, 48000, 9              # what dawn_resample16k_pcm16 refuses, under this entry's name
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0 and who in err() and "channels = 9" in err()
    m.channels = 2
    for rate in (999, 384001):
        assert L.dawn_generate_clip_media_rate(C.addressof(m), rate, WS, 1 << 20, None) != 0 and who in err() and f"rate = {rate}" in err()
    m.pcm = PCM + 1
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0 and "2-byte aligned" in err()
    m.pcm, m.n_frames = PCM, 2
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0 and "n_out = 0" in err()
    m.n_frames = 48000                                         # the media are fine now: the pipeline's own first refusal
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 48000, WS, 1 << 20, None) != 0 and who in err() and "NULL handle" in err()
    assert L.dawn_generate_media_rate_bytes(C.addressof(m), 48000, C.byref(cb), C.byref(wb)) != 0 and "NULL handle" in err()
    # 16000 is dawn_generate_clip_media: its refusals in its order, under this entry's name
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 16000, WS, 1 << 20, None) != 0 and who in err() and "NULL handle" in err()
    a.img3 = None
    assert L.dawn_generate_clip_media_rate(C.addressof(m), 16000, WS, 1 << 20, None) != 0 and "image is NULL" in err()
    assert (cb.value, wb.value) == (7, 7)


# ---------------------------------------------------------------------------------------------- the oracle, and audio.py under the gate
LD_BITS = np.finfo(np.longdouble).nmant


@pytest.mark.skipif(LD_BITS <= 52, reason="long double has no more mantissa than fp64 here")
@pytest.mark.parametrize("rate", [8000, 15999, 44100, 48000, 192000])
def test_oracle_equals_its_80_bit_evaluation(rate):
    """At most 2^-44 apart on full-scale random input: the oracle's own error sits far below the gate's absolute term (2^-40)."""
    pcm = pcm_for(rate, max(3 * rate // 100, 64), 1, seed=3)
    lo, hi = oracle(pcm, rate), oracle(pcm, rate, dtype=np.longdouble)
    d = float(np.abs(hi - lo.astype(np.longdouble)).max())
    print(f"rate {rate}: max|fp64 - 80-bit| = {d:.3e} over {lo.size} outputs")
    assert lo.size >= 4 and d <= 2.0 ** -44


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_audio_py_equals_the_oracle_under_the_gate(case):
    pcm, y64 = reference(case)
    got = audio.resample_to_16k(pcm if case[2] > 1 else pcm[:, 0], case[0])
    assert got.dtype == np.float32
    assert_gate(got, y64, f"audio.resample_to_16k {case_id(case)}")


def test_audio_py_fp32_input_16k_and_refusals():
    pcm, y64 = reference((44100, 3000, 2))
    x = (pcm[:, 0].astype(np.float32) / np.float32(32768))
    assert np.array_equal(audio.resample_to_16k(x, 44100), audio.resample_to_16k(pcm, 44100))
    assert np.array_equal(audio.resample_to_16k(pcm, 16000), pcm[:, 0].astype(np.float32) / np.float32(32768))
    for bad_rate in (999, 384001):
        with pytest.raises(ValueError, match="rate"):
            audio.resample_to_16k(pcm, bad_rate)
    with pytest.raises(ValueError, match="no output"):
        audio.resample_to_16k(pcm[:2], 48000)
    with pytest.raises(ValueError):
        audio.resample_to_16k(pcm.astype(np.int32), 48000)


def test_read_pcm16(tmp_path):
    def write(name, frames, rate, width=2):
        with wave.open(str(tmp_path / name), "wb") as f:
            f.setnchannels(frames.shape[1]); f.setsampwidth(width); f.setframerate(rate); f.writeframes(frames.tobytes())
        return str(tmp_path / name)
    for rate, ch in ((44100, 2), (8000, 1), (16000, 1), (48000, 6)):
        pcm = pcm_for(rate, 321, ch, seed=5)
        got = audio.read_pcm16(write(f"a{rate}_{ch}.wav", pcm, rate))
        assert got is not None and got[1] == rate and got[0].dtype == np.int16 and np.array_equal(got[0], pcm)
    assert audio.read_pcm16(write("b.wav", np.zeros((10, 1), dtype=np.uint8), 44100, width=1)) is None       # 8-bit PCM
    assert audio.read_pcm16(write("c.wav", np.zeros((0, 2), dtype=np.int16), 44100)) is None                 # no frame
    (tmp_path / "d.wav").write_bytes(b"not a wave file at all")
    assert audio.read_pcm16(str(tmp_path / "d.wav")) is None


def test_video_generator_audio_via_c_on_a_cpu_device_needs_no_ffmpeg(tmp_path, monkeypatch):
    """`VideoGenerator(audio_via_c=True)` on a CPU device: a stereo 22.05 kHz WAV goes through audio.resample_to_16k, with PATH emptied so
    that no ffmpeg can run.  The HuBERT object is a stand-in that hands its input back: the stage's input is what is checked."""
    import torch
    from dawn_pytorch_amd.video_generator import VideoGenerator

    class Echo:
        def process_audio(self, speech):
            return np.asarray(speech, dtype=np.float32)[:, None]
    pcm = pcm_for(22050, 1500, 2)
    with wave.open(str(tmp_path / "a.wav"), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(22050); f.writeframes(pcm.tobytes())
    vg = VideoGenerator.__new__(VideoGenerator)           # the stage needs no diffusion model
    vg.hubert, vg.audio_path, vg.frontend, vg.device = Echo(), str(tmp_path / "a.wav"), None, torch.device("cpu")
    vg.cache_path, vg.audio_emb_path = str(tmp_path), str(tmp_path / "target_audio.npy")
    vg.audio_via_c = True
    monkeypatch.setenv("PATH", "")
    vg.process_audio()
    got = np.load(vg.audio_emb_path)[:, 0]
    assert np.array_equal(got, audio.resample_to_16k(pcm, 22050))
    assert_gate(got, oracle(pcm, 22050), "VideoGenerator(audio_via_c=True), CPU device")
    vg.audio_via_c = False                                # the default path shells out for this file
    with pytest.raises((FileNotFoundError, OSError)):
        vg.process_audio()


# ---------------------------------------------------------------------------------------------- the filter
def tone_through(rate, f):
    """A unit tone of f Hz, 0.12 s at `rate`, through the oracle -> (interior outputs, their 16 kHz sample indices)."""
    x = np.sin(2 * np.pi * f * np.arange(int(0.12 * rate)) / rate)
    y = oracle(x, rate)
    i = np.arange(y.size)
    keep = slice(80, y.size - 80)                             # the filter's half width is at most 64 outputs
    return y[keep], i[keep]


def db(x):
    return 20 * np.log10(max(float(x), 1e-300))


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_pass_band_and_stop_band(rate):
    passed = [f for f in (100, 1000, 3000, 6000) if f < 0.75 * min(rate, 16000) / 2]
    stopped = [f for f in (8800, 10000, 15000, 20000) if f < rate / 2]
    assert passed
    for f in passed:
        y, i = tone_through(rate, f)
        A = np.stack((np.sin(2 * np.pi * f * i / 16000), np.cos(2 * np.pi * f * i / 16000)), 1)
        coef, *_ = np.linalg.lstsq(A, y, rcond=None)
        fit = A @ coef
        gain = db(np.hypot(*coef))
        resid = db(np.sqrt(np.mean((y - fit) ** 2)) / np.sqrt(np.mean(fit ** 2)))
        print(f"rate {rate}, {f} Hz: gain {gain:+.4f} dB, residual {resid:.1f} dB")
        assert abs(gain) <= 0.01 and resid <= -95, (rate, f, gain, resid)
    for f in stopped:
        y, _ = tone_through(rate, f)
        level = db(np.sqrt(np.mean(y ** 2)) / np.sqrt(0.5))
        print(f"rate {rate}, {f} Hz: output {level:.1f} dB")
        assert level <= -90, (rate, f, level)


# ---------------------------------------------------------------------------------------------- the gate rejects
def test_impulse_position_meets_the_last_tap():
    L, M, rho, W, K = plan(44100)
    q, r = divmod(489 * M, L)
    assert (q, r, K) == (1347, 129, 89) and q + K == IMPULSE_AT and abs(r / L - K) < W


@pytest.mark.parametrize("defect", ["drop_last_tap", "phase_plus_one", "K_minus_one", "position_fp32"])
def test_the_gate_rejects(defect):
    """On an impulse every output is one coefficient times 32767 / 32768, the table's tails included: a defect in one tap shows at the
    gate's absolute term.  The unmutated oracle, rounded to fp32, passes.  The impulse sits where the LAST tap of an output meets it with
    a non-zero coefficient: output 489 has (q, r) = divmod(489 * 441, 160) = (1347, 129), and r / 160 > 0.8 puts j = K = 89 inside W = 88.2."""
    pcm = impulse(3000, IMPULSE_AT)
    y64 = oracle(pcm, 44100)
    assert gate_excess(y64.astype(np.float32), y64)[0] <= 1.0
    bad = oracle(pcm, 44100, mutate=defect).astype(np.float32)
    excess, worst = gate_excess(bad, y64)
    print(f"{defect}: max error {worst:.3e}, {excess:.3g} x the gate")
    assert excess > 1.0, defect
