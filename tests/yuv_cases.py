"""The yuv420p ingest (csrc/yuv_ingest.hip, include/dawn_hip.h at dawn_yuv420_to_frames): an integer numpy restatement of the
conversion, the inputs of its tests and a .y4m writer.  Nothing here needs a GPU.

    C = Y - 16, D = U - 128, E = V - 128                       (D, E of the 2x2 block's one chroma sample)
    R = clamp8((298*C         + 409*E + 128) >> 8)
    G = clamp8((298*C - 100*D - 208*E + 128) >> 8)
    B = clamp8((298*C + 516*D         + 128) >> 8)             `>>` an arithmetic shift (numpy's on signed integers)"""
import numpy as np


def yuv_to_rgb(y, u, v):
    """Bytes (any shape, broadcast against each other) -> (..., 3) uint8, the definition above in int32 (|value| < 2^18)."""
    c = np.asarray(y, dtype=np.int32) - 16
    d = np.asarray(u, dtype=np.int32) - 128
    e = np.asarray(v, dtype=np.int32) - 128
    r = (298 * c + 409 * e + 128) >> 8
    g = (298 * c - 100 * d - 208 * e + 128) >> 8
    b = (298 * c + 516 * d + 128) >> 8
    return np.clip(np.stack(np.broadcast_arrays(r, g, b), -1), 0, 255).astype(np.uint8)


def planes(frames, H, W):
    """I420 frames (T, >= 3HW/2) uint8 -> Y (T,H,W), U, V (T,H/2,W/2)."""
    hw, q = H * W, (H // 2) * (W // 2)
    f = np.asarray(frames)
    return f[:, :hw].reshape(-1, H, W), f[:, hw:hw + q].reshape(-1, H // 2, W // 2), f[:, hw + q:hw + 2 * q].reshape(-1, H // 2, W // 2)


def frames_to_rgb(frames, H, W):
    """I420 frames (T, >= 3HW/2) uint8 (bytes past 3HW/2 of a row are padding) -> (T,H,W,3) uint8, chroma replicated over its block."""
    y, u, v = planes(frames, H, W)
    return yuv_to_rgb(y, u.repeat(2, 1).repeat(2, 2), v.repeat(2, 1).repeat(2, 2))


def random_frames(T, H, W, stride=None, seed=0, pad=0xAB):
    """(T, stride) uint8: every byte value with equal chance in the frames, `pad` in the bytes between them."""
    n = H * W * 3 // 2
    out = np.full((T, stride or n), pad, dtype=np.uint8)
    out[:, :n] = np.random.default_rng(seed).integers(0, 256, (T, n), dtype=np.uint8)
    return out


def exhaustive_frame():
    """One 4096 x 4096 I420 frame (1, 3 * 2^23) in which every (Y, U, V) triple occurs exactly once: chroma block (i, j), i, j < 2048,
    has k = 2048 i + j, (U, V) = (k & 255, (k >> 8) & 255) and the Y group g = k >> 16 (0 .. 63), whose four pixels hold Y = 4 g + 0 .. 3."""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    u, v, g = (k & 255).astype(np.uint8), ((k >> 8) & 255).astype(np.uint8), k >> 16
    y = np.empty((4096, 4096), dtype=np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[dy::2, dx::2] = 4 * g + 2 * dy + dx
    return np.concatenate((y.reshape(-1), u.reshape(-1), v.reshape(-1))).reshape(1, -1)


def y4m_bytes(frames, H, W, header=None, frame_header=b"FRAME\n"):
    """A YUV4MPEG2 stream of I420 frames (T, 3HW/2); `header` replaces the default stream header line (without its newline)."""
    head = (b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg" % (W, H)) if header is None else header
    return head + b"\n" + b"".join(frame_header + np.ascontiguousarray(f).tobytes() for f in np.asarray(frames))
