"""The model bundle file: the writer, the index reader and the checksum in numpy.  The C loader (csrc/dawn_bundle.hip, host parsing in
csrc/dawn_bundle_format.h) is the reader that counts; include/dawn_hip.h ("model bundle") is the definition, restated here.

One file, little-endian, every offset and size an unsigned 64-bit number, no compression, nothing optional.

    header, 64 bytes    0 magic b"DAWNBNDL"   8 u32 version = 1   12 u32 abi (dawn_abi_version() the struct blobs were written for)
                        16 u64 n_entries   24 u64 index_bytes   32 u64 payload_offset (multiple of 256)   40 u64 device_bytes (multiple
                        of 256)   48 u64 file_bytes   56 u64 zero
    index at byte 64    per entry 48 bytes + name:  0 u32 stage   4 u32 kind (0 device tensor, 1 host blob)   8 u32 dtype (informational)
                        12 u32 name_len   16 u64 offset from the payload start   24 u64 length   32 u64 s1   40 u64 s2   48 the name,
                        zero-padded to a multiple of 8 bytes
    payload             the device part [0, device_bytes): every tensor at a multiple of 256 bytes, zero-padded to a multiple of 4 bytes,
                        zeros between tensors -- it goes to the GPU as one region, a pointer is base + offset; then the host part:
                        blobs at multiples of 16 bytes.  "cfg" of a stage = the raw bytes of its cfg struct (the optional stage 7,
                        "motion": ctx.MotionCfg = dawn_motion_cfg; a loader from before it refuses a file that has it); in the stage "host":
                        "defaults" (Defaults = dawn_bundle_defaults), "steps.ddim.<S>" (S x ctx.DdimStep), "steps.ancestral.<S>"
                        (S x ctx.AncestralStep), made from the dicts of sampler.ddim_step_scalars / ancestral_step_scalars.
    checksum            an entry's bytes (a host blob zero-padded to whole words) as n little-endian 32-bit words w:
                        s1 = sum w[i] mod 2^64, s2 = sum (i + 1) w[i] mod 2^64.  An integrity check against truncated files, bad copies
                        and stale bundles; no protection against tampering.

A zero-length tensor is refused (by the writer and by the loader): no packer makes one, and its pointer would mean nothing.
The packers (pack.py, ctx.*_named_weights) stay the one definition of every packed layout: this module copies bytes."""
from __future__ import annotations

import ctypes as C
import struct
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

from .ctx import ClipMode

MAGIC = b"DAWNBNDL"
VERSION = 1
HEADER_BYTES, ENTRY_FIXED_BYTES, ALIGN, HOST_ALIGN = 64, 48, 256, 16
STAGES = ("hubert", "pose", "blink", "decoder", "inputs", "unet", "host", "motion")    # DAWN_STAGE_*: the order of PipelineEvaluator.ev, then host,
MODEL_STAGES = STAGES[:6] + STAGES[7:]      # then the optional motion-encode stage (7).  MODEL_STAGES: the ones with a weight table and a cfg
KIND_DEVICE, KIND_HOST = 0, 1
DTYPES = {"uint8": 0, "float32": 1, "bfloat16": 2, "float16": 3, "int32": 4, "float64": 5, "int64": 6, "int16": 7}
_M64 = (1 << 64) - 1


class Defaults(C.Structure):
    """Mirror of ``dawn_bundle_defaults``."""
    _fields_ = [("H", C.c_int), ("fea_ch", C.c_int), ("latent_dim", C.c_int), ("max_n_frames", C.c_int), ("sampling_step", C.c_int),
                ("ancestral", C.c_int), ("cond_scale", C.c_float),
                ("up_border", C.c_int), ("random_seed", C.c_uint64), ("mean", C.c_double * 3), ("bbox6", C.c_float * 6),
                ("init_pose6", C.c_float * 6), ("init_blink2", C.c_float * 2), ("clip", ClipMode)]


# VideoGenerator's fallbacks: the bbox of UVG:340-341, the init pose / blink of UVG:277-278, the yaml's shipped values
DEFAULTS = dict(H=256, fea_ch=272, latent_dim=256, max_n_frames=200, sampling_step=20, ancestral=0, cond_scale=1.0, up_border=0, random_seed=1234, mean=(0.0, 0.0, 0.0),
                bbox6=(64.0, 64.0, 192.0, 192.0, 256.0, 256.0), init_pose6=(0.0, 0.0, 0.0, 4.79e-04, 5.65e+01, 6.49e+01),
                init_blink2=(0.3, 0.3), clip_kind=0, clip_q=0.9)


def defaults_struct(**kw) -> Defaults:
    """DEFAULTS overridden by the keywords, as the struct."""
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"bundle defaults: unknown fields {sorted(unknown)}")
    v = {**DEFAULTS, **kw}
    d = Defaults()
    d.H, d.fea_ch, d.latent_dim, d.max_n_frames = int(v["H"]), int(v["fea_ch"]), int(v["latent_dim"]), int(v["max_n_frames"])
    d.sampling_step, d.ancestral = int(v["sampling_step"]), int(bool(v["ancestral"]))
    d.cond_scale, d.up_border, d.random_seed =float(v["cond_scale"]), int(v["up_border"]), int(v["random_seed"])
    d.mean = (C.c_double * 3)(*[float(x) for x in v["mean"]])
    d.bbox6 = (C.c_float * 6)(*[float(x) for x in v["bbox6"]])
    d.init_pose6 = (C.c_float * 6)(*[float(x) for x in v["init_pose6"]])
    d.init_blink2 = (C.c_float * 2)(*[float(x) for x in v["init_blink2"]])
    d.clip.kind, d.clip.q = int(v["clip_kind"]), float(v["clip_q"])
    return d


def checksum(buffer) -> Tuple[int, int]:
    """(s1, s2) of the bytes of `buffer` (anything with the buffer protocol), zero-padded to whole 32-bit words."""
    b = np.frombuffer(memoryview(buffer).cast("B"), dtype=np.uint8)
    if b.size % 4:
        b = np.concatenate((b, np.zeros(4 - b.size % 4, dtype=np.uint8)))
    w = b.view("<u4")
    s1 = s2 = 0
    step = 1 << 22
    for i0 in range(0, w.size, step):                       # uint64 arithmetic wraps mod 2^64, which is the definition
        c = w[i0:i0 + step].astype(np.uint64)
        idx = np.arange(i0 + 1, i0 + 1 + c.size, dtype=np.uint64)
        s1 = (s1 + int(np.add.reduce(c, dtype=np.uint64))) & _M64
        s2 = (s2 + int(np.add.reduce(idx * c, dtype=np.uint64))) & _M64
    return s1, s2


def _tensor_bytes(name: str, t) -> Tuple[np.ndarray, int]:
    """(the tensor's bytes as a uint8 array, dtype code); a torch tensor on any device is brought to the host as it is."""
    if isinstance(t, np.ndarray):
        a = np.ascontiguousarray(t)
        return a.reshape(-1).view(np.uint8), DTYPES.get(a.dtype.name, 0)
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"bundle tensor {name}: a torch tensor or a numpy array, not {type(t).__name__}")
    h = t.detach().contiguous().cpu().reshape(-1)
    return h.view(torch.uint8).numpy(), DTYPES.get(str(t.dtype).replace("torch.", ""), 0)


def _blob_bytes(name: str, v) -> bytes:
    if isinstance(v, (C.Structure, C.Array)):
        return bytes(v)
    if isinstance(v, (bytes, bytearray, memoryview)):
        return bytes(v)
    raise TypeError(f"bundle host blob {name}: bytes or a ctypes struct / array, not {type(v).__name__}")


def _up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def write_bundle(path, tables: Mapping[str, Mapping[str, object]], cfgs: Mapping[str, C.Structure], host: Mapping[str, object],
                 abi: Optional[int] = None) -> dict:
    """Write the file.  tables = {stage: {name: tensor}} (torch on any device, or numpy), cfgs = {stage: ctypes cfg struct},
    host = {name: bytes or ctypes struct / array} for the stage "host".  abi: the library's dawn_abi_version() unless given.
    One tensor is in host memory at a time.  Returns read_index(path)."""
    if abi is None:
        from . import _lib
        abi = int(_lib.lib().dawn_abi_version())
    for s in (*tables, *cfgs):
        if s not in MODEL_STAGES:
            raise ValueError(f"bundle: unknown stage {s!r} (one of {MODEL_STAGES})")
    dev = [(STAGES.index(s), str(n), t) for s in MODEL_STAGES if s in tables for n, t in tables[s].items()]
    blobs = [(STAGES.index(s), "cfg", _blob_bytes(f"{s}/cfg", cfgs[s])) for s in MODEL_STAGES if s in cfgs]
    blobs += [(6, str(n), _blob_bytes(str(n), v)) for n, v in host.items()]
    names = [(s, KIND_DEVICE, n) for s, n, _ in dev] + [(s, KIND_HOST, n) for s, n, _ in blobs]
    if len(set(names)) != len(names):
        raise ValueError("bundle: a name is given twice in a stage")
    for _, _, n in names:
        if not 1 <= len(n.encode()) <= 4096 or "\0" in n:
            raise ValueError(f"bundle: bad entry name {n!r}")
    index_bytes = sum(ENTRY_FIXED_BYTES + _up(len(n.encode()), 8) for _, _, n in names)
    payload_offset = _up(HEADER_BYTES + index_bytes, ALIGN)
    entries = []
    with open(path, "wb") as f:
        at = 0
        for s, n, t in dev:
            raw, code = _tensor_bytes(n, t)
            if raw.size == 0:
                raise ValueError(f"bundle: tensor {STAGES[s]}/{n} is empty (a zero-length tensor is refused)")
            pad = -raw.size % 4
            if pad:
                raw = np.concatenate((raw, np.zeros(pad, dtype=np.uint8)))
            s1, s2 = checksum(raw)
            f.seek(payload_offset + at)
            f.write(raw.data)
            entries.append((s, KIND_DEVICE, code, n, at, raw.size, s1, s2))
            at = _up(at + raw.size, ALIGN)
        device_bytes = at
        for s, n, b in blobs:
            if not b:
                raise ValueError(f"bundle: host blob {STAGES[s]}/{n} is empty")
            s1, s2 = checksum(b)
            f.seek(payload_offset + at)
            f.write(b)
            entries.append((s, KIND_HOST, 0, n, at, len(b), s1, s2))
            at = _up(at + len(b), HOST_ALIGN)
        file_bytes = payload_offset + at
        f.truncate(file_bytes)                              # (the gaps a seek skipped, the tail included, read as zeros)
        f.seek(0)
        f.write(MAGIC + struct.pack("<IIQQQQQQ", VERSION, abi, len(entries), index_bytes, payload_offset, device_bytes, file_bytes, 0))
        for s, kind, code, n, off, length, s1, s2 in entries:
            nb = n.encode()
            f.write(struct.pack("<IIIIQQQQ", s, kind, code, len(nb), off, length, s1, s2) + nb + b"\0" * (-len(nb) % 8))
        assert f.tell() == HEADER_BYTES + index_bytes
    return read_index(path)


def read_index(path) -> dict:
    """{"version", "abi", "n_entries", "index_bytes", "payload_offset", "device_bytes", "file_bytes", "entries": [{"stage", "kind",
    "dtype", "name", "offset", "length", "s1", "s2"}]} of the file -- the numbers as they stand; the C loader is what validates them."""
    with open(path, "rb") as f:
        head = f.read(HEADER_BYTES)
        if len(head) < HEADER_BYTES or head[:8] != MAGIC:
            raise ValueError(f"{path}: not a DAWN bundle")
        version, abi, n, index_bytes, payload_offset, device_bytes, file_bytes, _ = struct.unpack("<IIQQQQQQ", head[8:])
        index = f.read(index_bytes)
    out = dict(version=version, abi=abi, n_entries=n, index_bytes=index_bytes, payload_offset=payload_offset, device_bytes=device_bytes,
               file_bytes=file_bytes, entries=[])
    at = 0
    for _ in range(n):
        s, kind, code, nl, off, length, s1, s2 = struct.unpack_from("<IIIIQQQQ", index, at)
        name = index[at + ENTRY_FIXED_BYTES:at + ENTRY_FIXED_BYTES + nl].decode()
        out["entries"].append(dict(stage=STAGES[s] if s < len(STAGES) else s, kind=kind, dtype=code, name=name, offset=off, length=length,
                                   s1=s1, s2=s2))
        at += ENTRY_FIXED_BYTES + _up(nl, 8)
    return out


def steps_blob(name: str, steps: Sequence[dict]) -> C.Array:
    """The step dicts of sampler.ddim_step_scalars ("ddim.<S>") / ancestral_step_scalars ("ancestral.<S>") as the struct array."""
    from . import ctx
    kind = name.split(".")[0]
    if kind not in ("ddim", "ancestral") or name != f"{kind}.{len(steps)}":
        raise ValueError(f"bundle step table {name!r}: 'ddim.<S>' or 'ancestral.<S>' with S = the number of steps ({len(steps)})")
    cls = ctx.DdimStep if kind == "ddim" else ctx.AncestralStep
    arr = (cls * len(steps))()
    for i, st in enumerate(steps):
        for field, _ in cls._fields_:
            setattr(arr[i], field, st[field])
    return arr


def bundle_from_pipeline(path, pipe, steps: Mapping[str, Sequence[dict]], defaults: Optional[Mapping[str, object]] = None,
                         abi: Optional[int] = None, motion=None) -> dict:
    """The bundle of a ctx.PipelineEvaluator: the six evaluators' `weights` and `cfg`, exactly the tables _Evaluator.__init__ hands to
    *_create.  steps = {"ddim.20": ddim_step_scalars(...), "ancestral.1000": ...}; defaults = overrides of DEFAULTS (fea_ch, latent_dim
    and up_border are read off the evaluators).  motion = a motion_encoder.MotionEncoder or its ctx.MotionEvaluator: the optional
    seventh stage "motion" (ctx.motion_named_weights / ctx.motion_cfg), for dawn_bundle_create_motion."""
    tables = {s: ev.weights for s, ev in zip(STAGES, pipe.ev)}
    cfgs = {s: ev.cfg for s, ev in zip(STAGES, pipe.ev)}
    if motion is not None:
        from . import ctx
        if isinstance(motion, ctx.MotionEvaluator):
            if not motion.weights:
                raise ValueError("bundle: a MotionEvaluator that came from a bundle holds no weight table to write")
            tables["motion"], cfgs["motion"] = motion.weights, motion.cfg
        else:
            tables["motion"], cfgs["motion"] = ctx.motion_named_weights(motion), ctx.motion_cfg(motion)
    unet, pose = pipe.ev[5], pipe.ev[1]
    d = dict(fea_ch=unet.cfg.fea_ch, latent_dim=pose.cfg.latent_dim, up_border=int(getattr(getattr(unet, "P", None), "up_border", 0) or 0))
    if steps:                                               # the default step table: the first one given, unless the caller names one
        first = next(iter(steps))
        d.update(sampling_step=len(steps[first]), ancestral=first.startswith("ancestral."))
    d.update(defaults or {})
    host ={"defaults": defaults_struct(**d)}
    for name, st in steps.items():
        host[f"steps.{name}"] = steps_blob(name, st)
    return write_bundle(path, tables, cfgs, host, abi=abi)
