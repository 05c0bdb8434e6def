"""The resampler to 16 kHz (include/dawn_hip.h: dawn_resample16k_pcm16) as an oracle in numpy fp64, written from the definition and
independently of dawn_pytorch_amd/audio.py (no phase table: every coefficient is evaluated where it is used, and the taps are summed with
math.fsum, i.e. rounded once), the same in 80-bit long double, the case list and the gate.

THE GATE.  |got - y64| <= 2^-23 |y64| + 2^-40, derived, not measured:
  * 2^-23 |y64|: the implementation rounds its fp64 sum to fp32 once, 2^-24 |y| -- doubled;
  * 2^-40 (9.1e-13): the worst-case fp64 error of the longest filter the cases reach, 769 taps at 192 kHz: accumulation
    769 * 2^-53 * sum|x h| plus the coefficients' own error, about 3e-13 in total with |x| <= 1 and sum|h| < 3.
profiles/audio_resample.md records the largest observed error per case."""
import math

import numpy as np

Z, BETA, CUT = 32, 9.0, 0.92
REL, ABS = 2.0 ** -23, 2.0 ** -40

# (rate, n_frames, channels)
CASES = [(8000, 700, 1), (11025, 900, 2), (15999, 1200, 1), (22050, 1500, 1), (32000, 2000, 8), (44100, 3000, 2), (44101, 3000, 1),
         (48000, 3100, 1), (96000, 6000, 1), (192000, 9000, 1)]
SHORT = [(48000, 3, 1), (44100, 7, 1), (8000, 1, 1)]            # inputs shorter than the filter


def frames_for(n_out, rate):
    """The smallest n_frames with floor(n_frames * 16000 / rate) == n_out."""
    return -(-n_out * rate // 16000)


# n_out in {255, 256, 257}: one workgroup short of full, full, and one output into the second
EDGE = [(rate, frames_for(n_out, rate), 1) for rate in (48000, 44100) for n_out in (255, 256, 257)]
ALL_CASES = CASES + SHORT + EDGE
RATES = sorted({c[0] for c in ALL_CASES})


def case_id(c):
    return f"{c[0]}Hz-{c[1]}x{c[2]}"


def out_len(n_frames, rate):
    return n_frames * 16000 // rate if n_frames >= 1 and 1000 <= rate <= 384000 else 0


def table_bytes(rate):
    """dawn_resample16k_workspace_bytes: L rows of 2 K + 1 doubles, rounded up to 256 bytes."""
    if not 1000 <= rate <= 384000 or rate == 16000:
        return 0
    L = 16000 // math.gcd(16000, rate)
    return (L * (2 * plan(rate)[4] + 1) * 8 + 255) // 256 * 256


def pcm_for(rate, n_frames, channels, seed=0):
    """Seeded random int16 (n_frames, channels) that holds -32768 and 32767 in channel 0 (where there is room); the other channels are
    different noise, so that a wrong channel shows."""
    rng = np.random.default_rng([seed, rate, n_frames, channels])
    pcm = rng.integers(-32768, 32768, size=(n_frames, channels), dtype=np.int64).astype(np.int16)
    if n_frames >= 3:
        pcm[n_frames // 3, 0], pcm[2 * n_frames // 3, 0] = -32768, 32767
    elif n_frames == 1:
        pcm[0, 0] = -32768
    return pcm


IMPULSE_AT = 1436              # 4 * 359: at 44.1 kHz the last tap (j = K) of output 489 meets it inside the window (tests/test_resample_cpu.py)


def impulse(n_frames, at, channels=1):
    """One full-scale sample in channel 0, zeros elsewhere: every output is one coefficient times 32767 / 32768."""
    pcm = np.zeros((n_frames, channels), dtype=np.int16)
    pcm[at, 0] = 32767
    return pcm


def plan(rate):
    """(L, M, rho, W, K) of the definition; rho, W and K in fp64 -- they decide which taps exist."""
    g = math.gcd(16000, rate)
    rho = 1.0 if rate <= 16000 else 16000.0 / rate
    W = Z / rho
    return 16000 // g, rate // g, rho, W, int(math.ceil(W))


def i0(x, one=1.0):
    """sum_k ((x / 2)^k / k!)^2 of a scalar, in the type of `one`."""
    y = x / (one + one)
    p, s = one, one
    for k in range(1, 1000):
        p = p * y / (one * k)
        t = p * p
        s = s + t
        if t < (one * 2.0 ** -60) * s:
            break
    return s


def i0_vec(x, dtype):
    """The same series on an array: every element stops on its own term (a finished element no longer changes)."""
    y = x / dtype(2)
    p, s = np.ones_like(y), np.ones_like(y)
    live = np.ones(y.shape, dtype=bool)
    for k in range(1, 1000):
        p = p * y / dtype(k)
        t = p * p
        s = np.where(live, s + t, s)
        live &= t >= dtype(2.0 ** -60) * s
        if not live.any():
            break
    return s


PI_LD = np.longdouble(3.141592653589793) + np.longdouble(1.2246467991473532e-16)      # pi to the long double's precision


def h(u, rho, W, dtype=np.float64, inside=None):
    """The kernel function on an array u of `dtype`.  inside: which taps exist, where the caller has decided that already."""
    pi = PI_LD if dtype is np.longdouble else dtype(np.pi)
    rho_, W_, cut, beta = dtype(rho), dtype(W), dtype(CUT), dtype(BETA)
    t = rho_ * cut * u
    safe = np.where(t == 0, dtype(1), t)
    s = np.where(t == 0, dtype(1), np.sin(pi * safe) / (pi * safe))
    v = u / W_
    win = i0_vec(beta * np.sqrt(np.maximum(dtype(1) - v * v, dtype(0))), dtype) / i0(beta, dtype(1))
    return np.where(np.abs(u) < W_ if inside is None else inside, rho_ * cut * s * win, dtype(0))


def samples_of(x):
    """int16 (n,) / (n, ch) -> channel 0 / 32768; floating (n,) -> the fp32 values; both exact in fp64."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x[:, 0] if x.ndim == 2 else x).astype(np.float64) / 32768.0
    return x.astype(np.float32).astype(np.float64)


def oracle(x, rate, dtype=np.float64, mutate=None):
    """y (n_out,) of `dtype` by the definition.  fp64: the products are summed by math.fsum (exactly, rounded once).  long double: h, the
    products and an ascending sum in 80-bit, from the definition's fp64 rho, W and K and its fp64 decision |u| < W.
    mutate: a defect for the tests that show the gate rejects it -- "drop_last_tap", "phase_plus_one", "K_minus_one", "position_fp32"."""
    xs = samples_of(x)
    n = xs.shape[0]
    L, M, rho, W, K = plan(rate)
    n_out = out_len(n, rate)
    Kt = K - 1 if mutate == "K_minus_one" else K
    j = np.arange(-Kt, Kt + 1)
    if mutate == "drop_last_tap":
        j = j[:-1]
    jf = j.astype(dtype)
    xp = np.concatenate((np.zeros(K + 1), xs, np.zeros(K + 2)))          # xp[k + K + 1] = x[k]
    qr = [divmod(i * M, L) for i in range(n_out)]                         # Python integers: no overflow, no rounding
    q = np.array([a for a, _ in qr], dtype=np.int64)
    r = np.array([b for _, b in qr], dtype=np.int64)
    if mutate == "phase_plus_one":
        r = (r + 1) % L
    frac = r.astype(dtype) / dtype(L)
    if mutate == "position_fp32":                                         # the position as ONE fp32 number, then split again
        pos = np.arange(n_out, dtype=np.float32) * np.float32(rate) / np.float32(16000)
        fl = np.floor(pos)
        frac = (pos - fl).astype(dtype)
        q = np.clip(fl.astype(np.int64), 0, n)
    # |u| < W is decided in fp64, as the definition states it: at 44.1 kHz the phase r / L = 0.2 puts a tap exactly on the window's edge
    # W = 88.2, and the comparison of the two ROUNDED numbers is what every fp64 implementation reproduces
    inside = np.abs(frac.astype(np.float64)[:, None] - j.astype(np.float64)[None, :]) < W
    prod = xp[q[:, None] + j[None, :] + K + 1].astype(dtype) * h(frac[:, None] - jf[None, :], rho, W, dtype, inside)
    if dtype is np.float64:
        return np.array([math.fsum(row) for row in prod.tolist()], dtype=np.float64)
    y = np.zeros(n_out, dtype=dtype)
    for t in range(prod.shape[1]):                                        # ascending j
        y = y + prod[:, t]
    return y


_CACHE = {}


def reference(case):
    """(pcm, y64) of a case, computed once per session and shared (read-only)."""
    if case not in _CACHE:
        pcm = pcm_for(*case)
        y = oracle(pcm, case[0])
        pcm.setflags(write=False)
        y.setflags(write=False)
        _CACHE[case] = (pcm, y)
    return _CACHE[case]


def gate_excess(got, y64):
    """max over the outputs of |got - y64| / (2^-23 |y64| + 2^-40): <= 1 passes.  Also returns the largest absolute error."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - y64)
    return float((err / (REL * np.abs(y64) + ABS)).max()), float(err.max())


def assert_gate(got, y64, what=""):
    got = np.asarray(got)
    assert got.shape == y64.shape, (what, got.shape, y64.shape)
    assert np.isfinite(got).all(), what
    excess, worst = gate_excess(got, y64)
    print(f"{what}: max|got - y64| = {worst:.3e}, largest error / gate = {excess:.3f}")
    assert excess <= 1.0, (what, excess, worst)
