"""Guard bands and poison around the buffers of the UNet evaluation's kernels and of the stage and sampler kernels around it (flow decoder,
HuBERT, PBnet, sampler steps), for GPU op tests; shown to catch each defect on CPU tensors by tests/test_guarded_cpu.py.  A max-norm comparison of values cannot see three kinds of error:

  * an output element the kernel never wrote -- the results come from `torch.empty`, and the caching allocator hands the block
    of the previous, correct, call back: `GuardedOps.empty` fills every result with NaN first;
  * a write outside the output -- every result and every caller-supplied `out=` (`guarded_out`) lies between two row bands, and
    optionally between column neighbours, of a fixed bit pattern that `verify()` compares bit for bit;
  * a read outside an input that reaches the result -- `guarded_in` surrounds the input with NaN, which `0 * x` does not cancel.

Every band is part of ONE torch allocation that the helper owns: a stray access lands in owned memory and becomes an assertion.
Nothing here depends on the device: the same code carves CPU tensors.

What is guarded: what an op asks `HipOps.empty` / `conv_gn_part` for -- every result of every op of ops.py, the sampler ops, the frame
egress and the HuBERT ops included, and the private scratch `quantile_threshold.ws` that a histogram from elsewhere makes it allocate --
and what the test hands in through `guarded_out` / `guarded_in`.
NOT guarded: the three buffers ops.py still takes from torch directly, each cached for the life of the HipOps object and shared between calls,
so that no single call owns (or completely writes) it:
  * the per-clip table of `xattn_tables` (written once per clip, read by every evaluation);
  * the GroupNorm hand-off ticket of `_gn_ticket` (four words per (device, stream), zeroed by a stream-ordered fill);
  * the selection scratch `_sel_ws` of `ddim_x0` / `cfg_x0` / `quantile_threshold` (4104 words per (device, stream)) and the `hist` slice of
    it that `ddim_x0` and `cfg_x0` return: its contents are checked by value (the histogram is compared bin for bin with a bincount).

Byte outputs.  Poison is 0xFF and 255 is a legal RGB byte, so an integer payload is unambiguous only where the EXPECTED bytes hold no 255:
every guarded byte test first asserts that on its CPU reference (`assert_no_255`).  For I420 it holds by definition (Y <= 235, U and
V <= 240); for RGB the test draws its inputs so that the clipped value stays below 255/255 and keeps the mean at zero (the 255 level is pinned
by the byte-boundary tests of the egress, which are not guarded).  Under that condition the integer rule of `_poisoned` (== 255: never
written) is exact.

Outputs into a frame range of a longer clip (PARTIAL, below): the test guards the WHOLE clip, hands the op the frame-range view and states the
written rows, verify(written=...); every other row must still be poison.  For the fp32 clips (3, Ttot, H, W) the rows are the (channel,
frame) pairs: the clip is carved as (3 * Ttot, H * W).  A strided plane view as an INPUT (`grid`, a frame range of a (2, Ttot, h, w) clip) is
guarded as the whole clip too: the frames outside the range are ordinary in-buffer data that the value references would expose if read,
the bands around the whole clip are NaN.

Names.  A result is named `<HipOps method>.<variable it is assigned to>`, read off the calling line; a line that does not have that shape
is an error here, not a silent other name.  The names PARTIAL is keyed by are pinned twice: tests/test_guarded_cpu.py finds each in the
source of ops.py, and the GPU tests of those ops (tests/test_hip_guard.py, tests/test_hip_guard_stages.py) assert that the buffer of that
name was allocated.  A PARTIAL key whose variable is a parameter of its method names an output that only a caller supplies."""
import linecache
import re
import sys

import torch

from dawn_pytorch_amd.ops import HipOps

PATTERN = 0x7149F2CA          # the bands of every output, as int32 words.  fp32: ~1.0e30, fp64 (two words): ~1e238 -- finite, never NaN
POISON = -1                   # all-ones bytes: a NaN in fp32 and fp64, -1 / 255 in the integer dtypes
BAND_MIN_BYTES = 64 << 10
BAND_ROWS = 256

# Payloads that a correct launch leaves partly unwritten.  Everything that is not named here must be written completely.
# value = (reason, rule): rule(record) -> bool mask over the payload's dim 0 of the rows that MUST be written, or None = no row
# (scratch that the same call produces and consumes: only its bands are checked).  A caller that knows the rows states them:
# verify(written={name: rows}) -- those rows must be written AND the others must still be poison; without `written` the rule holds.
PARTIAL = {
    "conv_gn_part": ("dawn_conv_gemm_nblocks is an upper bound over every tile configuration; the launch reports the rows it wrote "
                     "(gn_part.dawn_rows) and the reduction reads those only",
                     lambda r: torch.arange(r.payload.shape[0]) < getattr(r.payload, "dawn_rows", r.payload.shape[0])),
    "sla_layer_c64.ws": ("scratch of the two-kernel layer: dawn_sla_ws_floats is an upper bound (slices x frames), produced and consumed "
                         "inside the same call", None),
    "head_out.out": ("one head at a time (hg or ho is None) writes that head's rows of the caller's `out` only",
                     lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),     # all three, unless the caller states the rows:
    # verify(written={"head_out.out": ...}); the rows it does not state must then still be poison
    # ---- outputs that a caller aims at a frame range of a longer clip: all rows, unless the caller states the frames it handed over
    "final_conv_blend.out_vid": ("a (3, T, H, W) frame-range view of a (3, Ttot, H, W) clip, carved as (3 * Ttot, H * W): only the (channel, frame) "
                                 "rows of the range are written", lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),
    "final_conv_blend.warped_vid": ("as final_conv_blend.out_vid", lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),
    "final_conv_blend_u8.frames": ("frames [t0, t1) of a (Ttot, H * W * 3) byte clip: only those frames are written",
                                   lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),
    "final_conv_blend_yuv420.frames": ("frames [t0, t1) of a (Ttot, 3 * H * W / 2) I420 clip: only those frames are written",
                                       lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),
    "frames_to_yuv420.out": ("the op's own allocation is written completely; a caller's `out` may be frames [t0, t1) of a longer I420 clip",
                             lambda r: torch.ones(r.payload.shape[0], dtype=torch.bool)),
}


# Every result that the stage and sampler ops of ops.py allocate (`<method>.<variable>`; the two step-tail entries share `_step_fixed`).
# tests/test_guarded_cpu.py finds each in the source of ops.py, tests/test_hip_guard_stages.py asserts that its launches allocated each.
STAGE_BUFFERS = (
    "affine_act.out", "bn_relu_pool2.out", "warp_blend.out", "frames_to_u8.out", "frames_to_yuv420.out",
    "wave_normalize.st", "wave_normalize.out", "hubert_conv0.out", "ln_affine_act.out", "add_act.out", "hubert_pos_conv.out", "attn64.out",
    "interp_linear.out", "attn_bias32.out",
    "ddim_x0.x0", "cfg_x0.eps", "cfg_x0.x0", "quantile_threshold.out", "quantile_threshold.ws", "ddim_update.x", "ancestral_update.out",
    "_step_fixed.out", "_step_fixed.x0", "cfg_combine.out", "philox_normal.out",
)


class GuardError(AssertionError):
    pass


def _round_up(n, m):
    return (n + m - 1) // m * m


class _Rec:
    """One carving: raw int32 words [front band | rows x width | back band]; the payload is columns [c0, c0 + cw) of every row."""

    def __init__(self, name, raw, band, rows, width, c0, cw, payload, fill, snap=None):
        self.name, self.raw, self.band, self.rows, self.width, self.c0, self.cw = name, raw, band, rows, width, c0, cw
        self.payload, self.fill, self.snap = payload, fill, snap

    def body(self):
        return self.raw[self.band:self.band + self.rows * self.width].view(self.rows, self.width)

    def surroundings(self):
        b = self.body()
        return (("front band (rows before the buffer)", self.raw[:self.band]),
                ("back band (rows after the buffer)", self.raw[self.band + self.rows * self.width:]),
                ("column neighbours on the left", b[:, :self.c0]),
                ("column neighbours on the right", b[:, self.c0 + self.cw:]))

    def check_surroundings(self, what):
        for where, t in self.surroundings():
            bad = t != self.fill
            if bool(bad.any()):
                idx = bad.nonzero()[0].tolist()
                raise GuardError(f"{self.name}: {what} -- {int(bad.sum())} 32-bit words of its {where} changed, the first at {idx}")


def _carve(name, shape, dtype, device, fill, col_pad=0):
    """-> _Rec whose payload has `shape` / `dtype`, poisoned; surroundings = `fill`."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    rows = shape[0] if len(shape) >= 2 else 1
    row_bytes = (numel // max(rows, 1)) * item
    assert not col_pad or (len(shape) == 2 and item >= 4), "column neighbours need 2-D rows of whole 32-bit words"
    if row_bytes % 4 or rows == 0:
        rows, row_bytes = 1, _round_up(numel * item, 4)          # flat: one row
    cw = row_bytes // 4
    c0 = col_pad * item // 4
    width = cw + 2 * c0
    band = _round_up(max(BAND_MIN_BYTES, BAND_ROWS * width * 4), 256) // 4
    raw = torch.full((2 * band + rows * width,), fill, dtype=torch.int32, device=device)
    body = raw[band:band + rows * width].view(rows, width)
    body[:, c0:c0 + cw] = POISON
    if col_pad:
        payload = body.view(dtype)[:, col_pad:col_pad + shape[1]]
    else:
        payload = raw[band:band + rows * width].view(dtype)[:numel].view(shape)
    return _Rec(name, raw, band, rows, width, c0, cw, payload, fill)


def _poisoned(t):
    """bool tensor like t: the element still holds poison (float: any NaN -- also what a NaN that was read turns a result into; integer:
    all-ones, which for bytes is exact only under the condition of the module docstring: the expected bytes hold no 255)."""
    return torch.isnan(t) if t.dtype.is_floating_point else t == torch.tensor(POISON).to(t.dtype)


def _call_site():
    """`<HipOps method>.<assigned variable>` of the line that asked for the buffer (e.g. `sla_layer_c64.ws`, `conv_gemm.out`)."""
    f = sys._getframe(2)
    line = linecache.getline(f.f_code.co_filename, f.f_lineno)
    m = re.match(r"\s*(\w+)\s*=[^=]", line)
    if not m:
        raise GuardError(f"{f.f_code.co_filename}:{f.f_lineno}: cannot name the buffer asked for here (expected `name = ...empty(...)` on one line): "
                         f"{line.strip()!r}")
    return f"{f.f_code.co_name}.{m.group(1)}"


def assert_no_255(want):
    """The precondition of every guarded byte test (module docstring), on the CPU reference: no expected byte equals the poison."""
    want = torch.as_tensor(want)
    assert want.dtype == torch.uint8 and not bool((want == 255).any()), "a guarded byte test needs expected bytes below 255 (255 is the poison)"


class GuardedOps(HipOps):
    """HipOps whose every result is carved out of a guarded, poisoned allocation; see the module docstring."""

    def __init__(self, comm=None, device=None):
        super().__init__(comm)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.outs = []          # live carvings of results and caller-supplied outputs
        self.ins = []           # guarded inputs

    # ------------------------------------------------------------------ allocation
    def empty(self, *shape, like=None, dtype=torch.float32, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        r = _carve(_call_site(), shape, dtype, like.device if like is not None else device, PATTERN)
        self.outs.append(r)
        return r.payload

    def conv_gn_part(self, rows_out, N, like):
        r = _carve("conv_gn_part", (self.L.dawn_conv_gemm_nblocks(rows_out, N), 16), torch.float64, like.device, PATTERN)
        self.outs.append(r)
        return r.payload

    def guarded_out(self, rows, N, col_pad=0, *, name="out", dtype=torch.float32):
        """A caller-supplied `out=`: (rows, N), poisoned, between row bands; col_pad > 0: a column slice of a (rows, N + 2*col_pad)
        tensor of the pattern, so that ld_out > N."""
        r = _carve(name, (rows, N), dtype, self.device, PATTERN, col_pad)
        self.outs.append(r)
        return r.payload

    def guarded_in(self, t, col_pad=0, *, name="in"):
        """Copy of the (CPU) tensor t on the device, between row bands -- and with col_pad column neighbours -- of NaN.
        -> (view, bitwise snapshot of the view as int32 words)."""
        t = t.contiguous()
        r = _carve(name, t.shape, t.dtype, self.device, POISON, col_pad)
        r.payload.copy_(t)
        r.snap = r.body()[:, r.c0:r.c0 + r.cw].clone()
        self.ins.append(r)
        return r.payload, r.snap

    def reset(self):
        self.outs, self.ins = [], []

    # ------------------------------------------------------------------ checks
    def verify(self, written=None):
        """Every band bit-identical to the pattern, every payload free of poison.  written = {name: rows (slice / index / bool mask over
        dim 0)} for the buffers of PARTIAL whose rows the caller states: those rows must be written and the others still poison."""
        written = dict(written or {})
        for name in written:
            if name not in PARTIAL:
                raise GuardError(f"{name}: not in guarded.PARTIAL -- a buffer that is not listed there must be written completely")
        for r in self.outs:
            r.check_surroundings("write outside the buffer")
            bad = _poisoned(r.payload)
            if r.name in PARTIAL:
                need = torch.zeros(r.payload.shape[0], dtype=torch.bool)
                if r.name in written:
                    need[written[r.name]] = True
                    keep = bad.reshape(bad.shape[0], -1)[(~need).to(bad.device)]
                    if not bool(keep.all()):
                        raise GuardError(f"{r.name}: rows outside the stated written part were written ({int((~keep).sum())} elements)")
                elif PARTIAL[r.name][1] is not None:
                    need = PARTIAL[r.name][1](r)
                bad = bad[need.to(bad.device)]
            if bool(bad.any()):
                idx = bad.nonzero()[0].tolist()
                hint = (f" ({r.name} is in guarded.PARTIAL: a call that writes only some of its rows states them, verify(written={{{r.name!r}: rows}}))"
                        if r.name in PARTIAL and r.name not in written else "")
                raise GuardError(f"{r.name}: {int(bad.sum())} of {bad.numel()} elements hold poison (NaN) -- never written, or computed from "
                                 f"a NaN read outside an input; the first at {idx}{hint}")

    def inputs_intact(self, overwritten=()):
        """Every guarded input, its bands and neighbours, bit-identical to what guarded_in left; `overwritten` names the operands an
        in-place call writes over (their surroundings are still checked)."""
        names = {r.name for r in self.ins}
        for n in overwritten:
            if n not in names:
                raise GuardError(f"{n}: named as overwritten, but no guarded input has that name")
        for r in self.ins:
            r.check_surroundings("write outside the input")
            if r.name in overwritten:
                continue
            bad = r.body()[:, r.c0:r.c0 + r.cw] != r.snap
            if bool(bad.any()):
                idx = bad.nonzero()[0].tolist()
                raise GuardError(f"{r.name}: input modified -- {int(bad.sum())} 32-bit words differ from the snapshot, the first at {idx}")
