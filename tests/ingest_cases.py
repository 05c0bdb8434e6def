"""Cases, inputs and the integer restatement for the media-ingest tests (tests/test_ingest_cpu.py, tests/test_hip_ingest.py) and for
tools/gen_goldens_ingest.py, which writes tests/golden/image_ingest.npz with the installed Pillow.

Inputs come from a formula (no committed image, no random stream); the goldens hold the expected OUTPUT bytes only.  `resample_u8` is
include/dawn_hip.h's statement of dawn_image_ingest in plain Python doubles (no fused multiply-add) and int64 sums."""
import numpy as np

# name -> (Hs, Ws, Ho, Wo, input): the smallest shape at which each failure mode exists
CASES = {
    "identity": (8, 8, 8, 8, "formula"),                    # a skipped pass run with weights; layout and / 255 only
    "one_pixel": (1, 1, 4, 4, "formula"),                   # both clamps at once, a single tap
    "upscale": (5, 7, 8, 8, "formula"),                     # support 1, edge windows cut by the clamps, 1-2 taps
    "ragged_out": (9, 13, 6, 10, "formula"),                # output width no multiple of 4, odd plane size
    "fractional_shrink": (37, 23, 8, 8, "formula"),         # non-integer scale, window length varying by output
    "horizontal_only": (8, 50, 8, 12, "formula"),           # vertical pass skipped
    "vertical_only": (50, 8, 12, 8, "formula"),             # horizontal pass skipped
    "long_support": (200, 301, 4, 4, "formula"),            # 101-151 taps: past a 64- / 128-tap tile; fp64 sum order; FMA contraction
    "very_long_support": (2160, 3840, 8, 8, "formula"),     # 541- / 961-tap windows, int32 accumulator, rows-needed logic
    "near_unit_scale": (257, 255, 256, 256, "formula"),     # one axis shrinks, the other grows
    "workload_150": (150, 150, 32, 32, "formula"),          # the sizes the end-to-end tests feed
    "workload_80": (80, 80, 32, 32, "formula"),
    "saturating_p1_down": (24, 24, 8, 8, "checker1"),       # rounding at .5, clip at 0 and 255
    "saturating_p1_up": (24, 24, 32, 32, "checker1"),
    "saturating_p3_down": (24, 24, 8, 8, "checker3"),
    "saturating_p3_up": (24, 24, 32, 32, "checker3"),
}
# parts of an output that the golden keeps (a case not named here keeps all of it): name -> {part: (row slice, column slice)}
PARTS = {"near_unit_scale": {"corner": (slice(0, 32), slice(0, 32)), "last_rows": (slice(-8, None), slice(None)),
                             "last_cols": (slice(None), slice(-8, None))}}
PASS_ORDER_SHAPE = (1023, 3, 8, 8)          # where Pillow 12.2.0 was seen to run the vertical pass first


def formula(Hs, Ws, C=3, xp=np, **kw):
    """v(y, x, c) = (131 y + 71 x + 29 c + (y x) % 251) % 256 as (Hs, Ws, C) integers -- numpy here; xp = torch, device="cuda" makes it
    on the device."""
    y, x, c = xp.arange(Hs, **kw).reshape(-1, 1, 1), xp.arange(Ws, **kw).reshape(1, -1, 1), xp.arange(C, **kw).reshape(1, 1, -1)
    return (131 * y + 71 * x + 29 * c + (y * x) % 251) % 256


def checker(Hs, Ws, period):
    """0 / 255 checkerboard with squares of `period` pixels, the three channels in different phases."""
    y, x, c = np.arange(Hs).reshape(-1, 1, 1), np.arange(Ws).reshape(1, -1, 1), np.arange(3).reshape(1, 1, -1)
    return (((y // period + x // period + c) % 2) * 255).astype(np.uint8)


def source(name):
    Hs, Ws, _, _, kind = CASES[name]
    return formula(Hs, Ws).astype(np.uint8) if kind == "formula" else checker(Hs, Ws, int(kind[-1]))


def parts_of(name, out):
    """{key of the golden file: array} for an (Ho, Wo, ...) output of the case."""
    if name not in PARTS:
        return {name: out}
    return {f"{name}/{part}": out[rows, cols] for part, (rows, cols) in PARTS[name].items()}


def coeffs(n, m):
    """[(lo, [k ...])] for every output index: Pillow's precompute_coeffs (bilinear) + normalize_coeffs_8bpc."""
    scale = float(n) / float(m)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    table = []
    for i in range(m):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n)
        w = []
        for j in range(hi - lo):
            t = abs((j + lo - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        table.append((lo, [int(0.5 + (v / ww) * 4194304.0) for v in w]))
    return table


def _pass(a, m, axis):
    """One pass along `axis` of the uint8 array `a` to length m; bytes out."""
    n = a.shape[axis]
    if n == m:
        return a                                            # skipped, not run with unit weights
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((m,) + a.shape[1:], dtype=np.int64)
    for i, (lo, k) in enumerate(coeffs(n, m)):
        acc = np.tensordot(np.asarray(k, dtype=np.int64), a[lo:lo + len(k)], axes=(0, 0)) + (1 << 21)
        assert int(acc.max()) < 2 ** 31                     # the kernel's accumulator is int32
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resample_u8(a, Ho, Wo, order="hv"):
    """(Hs, Ws[, C]) uint8 -> (Ho, Wo[, C]) uint8; "hv" = horizontal pass first (the entry point's contract), "vh" = vertical first."""
    for ax in order:
        a = _pass(a, Wo if ax == "h" else Ho, 1 if ax == "h" else 0)
    return a
