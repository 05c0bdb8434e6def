"""Audio input without ffmpeg: a 16-bit PCM WAV of any sample rate read with the standard library, and the resampler to 16 kHz that
csrc/audio_resample.hip runs on the GPU, stated here in numpy fp64 for hosts without one.

The resampler is DEFINED in include/dawn_hip.h (dawn_resample16k_pcm16): a polyphase Kaiser-windowed sinc, Z = 32 zero crossings per
side, BETA = 9, CUT = 0.92.  Its values are that definition's, not ffmpeg's (swresample's output depends on build and version); nobody
has measured what the difference does to the HuBERT features."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

Z, BETA, CUT = 32, 9.0, 0.92
MIN_RATE, MAX_RATE = 1000, 384000


def read_pcm16(path: str) -> Optional[Tuple[np.ndarray, int]]:
    """(int16 frames (n_frames, channels), sample rate) of a 16-bit PCM WAV with 1 .. 8 channels, read with the stdlib; None for any
    other file."""
    import wave
    try:
        with wave.open(path, "rb") as f:
            sr, nch, sw, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
    except (wave.Error, EOFError):
        return None
    if sw != 2 or not 1 <= nch <= 8 or len(raw) < 2 * nch:
        return None
    return np.frombuffer(raw, dtype="<i2").reshape(-1, nch).copy(), int(sr)


def resample_len(n_frames: int, rate: int) -> int:
    """dawn_resample16k_len: floor(n_frames * 16000 / rate); 0 where the call would be refused."""
    if n_frames < 1 or n_frames > 1 << 34 or not MIN_RATE <= rate <= MAX_RATE:
        return 0
    return n_frames * 16000 // rate


def _i0(x: np.ndarray) -> np.ndarray:
    """sum_k ((x / 2)^k / k!)^2, every element summed until its term falls below 2^-60 of its sum."""
    y = np.asarray(x, dtype=np.float64) / 2.0
    p, total = np.ones_like(y), np.ones_like(y)
    live = np.ones(y.shape, dtype=bool)
    for k in range(1, 1000):
        p = p * y / float(k)
        term = p * p
        total = np.where(live, total + term, total)
        live &= ~(term < 2.0 ** -60 * total)
        if not live.any():
            break
    return total


def phase_rows(rate: int, rows: np.ndarray) -> Tuple[np.ndarray, int]:
    """(coef[rows], K): the rows `rows` of the definition's phase table for `rate`, each 2 K + 1 fp64 values."""
    g = math.gcd(16000, rate)
    L = 16000 // g
    rho = 1.0 if rate <= 16000 else 16000.0 / rate
    W = Z / rho
    K = int(math.ceil(W))
    j = np.arange(-K, K + 1, dtype=np.float64)
    u = (np.asarray(rows, dtype=np.float64) / float(L))[:, None] - j[None, :]
    t = rho * CUT * u
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    v = u / W
    win = _i0(BETA * np.sqrt(np.maximum(1.0 - v * v, 0.0))) / float(_i0(np.float64(BETA)))
    return np.where(np.abs(u) < W, rho * CUT * s * win, 0.0), K


def resample_to_16k(x: np.ndarray, rate: int) -> np.ndarray:
    """int16 (n,) / (n, channels) -- channel 0, / 32768 -- or floating (n,) samples at `rate` -> float32 samples at 16 kHz, by the
    definition: fp64 taps in ascending order, one rounding to fp32, no clipping.  rate == 16000 is the conversion alone."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = (x[:, 0] if x.ndim == 2 else x).astype(np.float64) / 32768.0
    elif x.ndim == 1 and x.dtype.kind == "f":
        x = x.astype(np.float32).astype(np.float64)            # the fp32 entry's input
    else:
        raise ValueError("resample_to_16k: int16 (n[, channels]) or floating (n,) samples")
    if x.ndim != 1:
        raise ValueError("resample_to_16k: int16 (n[, channels]) or floating (n,) samples")
    n = int(x.shape[0])
    if not MIN_RATE <= rate <= MAX_RATE:
        raise ValueError(f"resample_to_16k: rate = {rate}: {MIN_RATE} .. {MAX_RATE}")
    if rate == 16000:
        return x.astype(np.float32)
    n_out = resample_len(n, rate)
    if n_out < 1:
        raise ValueError(f"resample_to_16k: n_frames = {n} at rate = {rate} yields no output sample")
    g = math.gcd(16000, rate)
    L, M = 16000 // g, rate // g
    pos = np.arange(n_out, dtype=np.int64) * M                 # never a floating-point position
    q, r = pos // L, pos % L
    used, row_of = np.unique(r, return_inverse=True)           # only the table rows this signal visits
    coef, K = phase_rows(rate, used)
    xp = np.concatenate((np.zeros(K), x, np.zeros(K + 1)))     # xp[k + K] = x[k], zeros outside the signal
    q = np.minimum(q, n)                                       # (q <= n - 1 + (L - 1) / L already: a no-op that bounds the index)
    y = np.zeros(n_out, dtype=np.float64)
    for t in range(2 * K + 1):                                 # j = t - K ascending
        y += xp[q + t] * coef[row_of, t]
    return y.astype(np.float32)
