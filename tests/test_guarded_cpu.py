"""tests/guarded.py catches what it is for, shown on CPU tensors: an op with each defect planted is rejected with a message that
names the buffer, and the correct op passes.  A GPU test built on the helper proves something only because of this."""
import pytest
import torch

from guarded import PARTIAL, PATTERN, GuardedOps, GuardError


class FakeOps(GuardedOps):
    """`scale2`: out = 2 * x on (rows, C) views with a row stride, written the way a tiled kernel would -- and wrong on request."""

    def scale2(self, x, out=None, defect=None):
        rows, C = x.shape
        if out is None:
            out = self.empty(rows, C, like=x)
        for r in range(rows):
            if defect == "skip_row" and r == rows - 1:
                continue                                                      # the ragged last row tile
            for c0 in range(0, C, 16):
                if defect == "skip_col_tile" and c0 == 16:
                    continue
                out[r, c0:c0 + 16] = 2 * x[r, c0:c0 + 16]
        if defect == "row_past_end":
            torch.as_strided(out, (rows + 1, C), out.stride(), out.storage_offset())[rows] = 1.0
        if defect == "col_left_of_slice":
            torch.as_strided(out, (rows, 1), out.stride(), out.storage_offset() - 1)[3] = 1.0
        if defect == "overread_times_zero":                                   # a fetch clamped past the end, "cancelled" by a zero weight
            past = torch.as_strided(x, (rows + 1, C), x.stride(), x.storage_offset())[rows]
            out[0] += 0.0 * past
        if defect == "writes_input":
            x[1, 2] = 5.0
        return out


ROWS, C = 37, 48


@pytest.fixture
def g():
    return FakeOps(device="cpu")


def _run(g, defect, col_pad=0, own_out=False):
    x = torch.arange(ROWS * C, dtype=torch.float32).reshape(ROWS, C)
    xg, snap = g.guarded_in(x, col_pad, name="x")
    assert torch.equal(xg, x) and snap.dtype == torch.int32 and xg.stride(0) == C + 2 * col_pad
    out = g.guarded_out(ROWS, C, col_pad, name="y3_slice") if own_out else None
    got = g.scale2(xg, out=out, defect=defect)
    assert got.stride(0) == C + 2 * (col_pad if own_out else 0)
    return got, 2 * x


@pytest.mark.parametrize("col_pad,own_out", [(0, False), (8, False), (0, True), (8, True)])
def test_correct_op_passes(g, col_pad, own_out):
    got, want = _run(g, None, col_pad, own_out)
    g.verify()
    g.inputs_intact()
    assert torch.equal(got, want)


@pytest.mark.parametrize("defect,col_pad,own_out,buffer,words", [
    ("skip_row", 0, False, "scale2.out", "never written"),
    ("skip_col_tile", 0, False, "scale2.out", "never written"),
    ("skip_col_tile", 8, True, "y3_slice", "never written"),
    ("row_past_end", 0, False, "scale2.out", "back band"),
    ("row_past_end", 8, True, "y3_slice", "back band"),
    ("col_left_of_slice", 8, True, "y3_slice", "column neighbours on the left"),
    ("overread_times_zero", 0, False, "scale2.out", "NaN read outside an input"),
    ("overread_times_zero", 8, False, "scale2.out", "NaN read outside an input"),
])
def test_planted_defect_is_rejected(g, defect, col_pad, own_out, buffer, words):
    _run(g, defect, col_pad, own_out)
    with pytest.raises(GuardError) as e:
        g.verify()
    assert str(e.value).startswith(buffer + ":") and words in str(e.value), str(e.value)
    g.inputs_intact()                                    # (none of these touches its input)


def test_values_alone_would_not_have_noticed():
    """Why the poison is needed: into a buffer that still holds the previous correct answer the skipped row `passes`."""
    x = torch.arange(ROWS * C, dtype=torch.float32).reshape(ROWS, C)
    stale = 2 * x
    got = FakeOps(device="cpu").scale2(x, out=stale.clone(), defect="skip_row")
    assert torch.equal(got, 2 * x)


def test_modified_input_is_rejected_unless_named(g):
    _run(g, "writes_input")
    g.verify()
    with pytest.raises(GuardError, match=r"^x: input modified"):
        g.inputs_intact()
    g.inputs_intact(overwritten=("x",))                  # an in-place call names the operand it overwrites
    with pytest.raises(GuardError, match="no guarded input"):
        g.inputs_intact(overwritten=("y",))


def test_write_into_an_inputs_band_is_rejected_even_when_overwritten(g):
    x, _ = g.guarded_in(torch.ones(5, 8), name="x")
    torch.as_strided(x, (1, 8), x.stride(), x.storage_offset() - 8)[0] = 0.0
    with pytest.raises(GuardError, match=r"^x: write outside the input.*front band"):
        g.inputs_intact(overwritten=("x",))


def test_layout_band_size_alignment_and_fill(g):
    like = torch.zeros(1)
    for shape, dtype, band_bytes in (((10, 64), torch.float32, 65536), ((10, 768), torch.float32, 256 * 768 * 4),
                                     ((7, 16), torch.float64, 65536), ((5,), torch.float32, 65536), ((3, 5), torch.uint8, 65536)):
        t = g.empty(*shape, like=like, dtype=dtype)
        r = g.outs[-1]
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert r.band * 4 == band_bytes and r.band * 4 % 256 == 0
        assert (t.data_ptr() - r.raw.data_ptr()) == r.band * 4                # the payload is as aligned as the allocation + 256 B
        assert bool((r.raw[:r.band] == PATTERN).all()) and bool((r.raw[-r.band:] == PATTERN).all())
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        else:
            assert bool((t == 255).all())
        assert r.name == "test_layout_band_size_alignment_and_fill.t"        # the call site names the buffer
    assert not torch.isnan(torch.tensor([PATTERN], dtype=torch.int32).view(torch.float32)).any()
    assert not torch.isnan(torch.tensor([PATTERN, PATTERN], dtype=torch.int32).view(torch.float64)).any()
    with pytest.raises(GuardError, match="never written"):
        g.verify()


def test_partial_buffers_only_by_the_table(g):
    like = torch.zeros(1)
    part = g.conv_gn_part(64, 64, like)                  # rows beyond dawn_rows may stay unwritten ...
    part[:2] = 0.0
    part.dawn_rows = 2
    g.verify()
    part.dawn_rows = 3                                   # ... the reported ones may not
    with pytest.raises(GuardError, match=r"^conv_gn_part: .*never written"):
        g.verify()
    g.reset()
    out = g.guarded_out(3, 20, name="head_out.out")
    out[:2] = 1.0
    g.verify(written={"head_out.out": slice(0, 2)})
    with pytest.raises(GuardError, match=r"^head_out.out: .*never written"):
        g.verify(written={"head_out.out": slice(0, 3)})
    with pytest.raises(GuardError, match=r"^head_out.out: rows outside the stated written part"):
        g.verify(written={"head_out.out": slice(0, 1)})
    with pytest.raises(GuardError, match="not in guarded.PARTIAL"):
        g.verify(written={"out": slice(0, 1)})
    assert all(reason for reason, _ in PARTIAL.values())


def test_partial_names_exist_in_ops():
    """The exemptions are keyed by `<method>.<variable>` read off the line in ops.py that asks for the buffer.  A rename or a re-flowed call
    there must not let an exemption lapse, or start to apply to another buffer, unnoticed: every key is found in the source of its method,
    assigned on one line from self.empty(...) -- or is the method that GuardedOps overrides."""
    import inspect
    import re
    from dawn_pytorch_amd.ops import HipOps
    for key in PARTIAL:
        if "." not in key:
            assert callable(getattr(HipOps, key)) and key in GuardedOps.__dict__, key
            continue
        method, var = key.split(".")
        src = inspect.getsource(getattr(HipOps, method))
        if var in inspect.signature(getattr(HipOps, method)).parameters and f"{var} = self.empty(" not in src:
            continue                                     # an output that only a caller supplies: the parameter of that name
        assert len(re.findall(rf"^\s*{var} = self\.empty\(.*\)$", src, re.M)) == 1, key


def test_stage_buffer_names_exist_in_ops():
    """Every name of guarded.STAGE_BUFFERS is a result that its method of ops.py asks self.empty for, on one line (guarded._call_site reads
    the name off that line) -- and ops.py takes nothing else from torch directly but the three cached buffers the guarded.py docstring
    lists."""
    import inspect
    import re
    from dawn_pytorch_amd import ops
    from guarded import STAGE_BUFFERS
    assert len(set(STAGE_BUFFERS)) == len(STAGE_BUFFERS)
    for key in STAGE_BUFFERS:
        method, var = key.split(".")
        src = inspect.getsource(getattr(ops.HipOps, method))
        assert len(re.findall(rf"^\s*{var} = self\.empty\(.*\)$", src, re.M)) == 1, key
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_guard_stages.py")) as f:
        gpu_tests = f.read()
    for key in STAGE_BUFFERS:                            # ... and the GPU tests assert that a launch allocated it (finish(alloc=...))
        assert f'"{key}"' in gpu_tests, key
    direct = re.findall(r"^.*torch\.(?:empty|zeros|full|empty_like|zeros_like)\(.*$", inspect.getsource(ops), re.M)
    left = [ln.strip() for ln in direct if not ln.strip().startswith("return torch.empty(")]          # (HipOps.empty / conv_gn_part themselves)
    assert len(left) == 4 and sum("_sel_ws[key]" in ln for ln in left) == 2 and sum("_tickets[key]" in ln for ln in left) == 1 \
        and sum(ln.startswith("xtab = ") for ln in left) == 1, left


# ---------------------------------------------------------------------------------------------- the stage and sampler kernels' hazards
class StageFake(GuardedOps):
    """The access patterns of the stage and sampler kernels on CPU tensors, each wrong on request: a 128-bit body with a scalar tail, rows
    stored into a frame range of a longer clip, a 128-bit load, a byte output."""

    def step4(self, x, defect=None):
        """out = x + 1 over n floats: n // 4 four-element accesses, then the n % 4 tail."""
        n = x.numel()
        out = self.empty(n, like=x)
        for i in range(0, n - n % 4, 4):
            out[i:i + 4] = x[i:i + 4] + 1
        if defect != "drop_tail":
            out[n - n % 4:] = x[n - n % 4:] + 1
        if defect == "read_4_bytes_before":               # the first 128-bit load starts one float early; its stray lane is "weighted by zero"
            v = torch.as_strided(x, (4,), (1,), x.storage_offset() - 1)
            out[0] += 0.0 * v[0]
        return out

    def fill_frames(self, frames, defect=None):
        """frames (T, N): a frame range of a longer clip; every row := 1."""
        T, N = frames.shape
        frames[:] = 1
        if defect == "row_past_range":
            torch.as_strided(frames, (T + 1, N), frames.stride(), frames.storage_offset())[T] = 1
        return frames

    def to_bytes(self, x, defect=None):
        out = self.empty(x.shape[0], x.shape[1], 3, like=x, dtype=torch.uint8)
        out[:] = (x.clamp(0, 1) * 254)[..., None].to(torch.uint8)
        if defect == "one_byte_unwritten":
            out[2, 1, 2] = 255                            # (what the poison left there)
        return out


@pytest.fixture
def sg():
    return StageFake(device="cpu")


@pytest.mark.parametrize("n", [3, 4, 7, 1027])
def test_dropped_tail_and_early_128_bit_read_are_rejected(sg, n):
    x = torch.arange(n, dtype=torch.float32)
    for defect, words in ((None, None), ("drop_tail", "never written"), ("read_4_bytes_before", "NaN read outside an input")):
        sg.reset()
        got = sg.step4(sg.guarded_in(x, name="x")[0], defect)
        if words is None or (defect == "drop_tail" and n % 4 == 0):
            sg.verify()
            assert torch.equal(got, x + 1)
        else:
            with pytest.raises(GuardError) as e:
                sg.verify()
            assert str(e.value).startswith("step4.out:") and words in str(e.value), str(e.value)
            if defect == "drop_tail":
                assert f"{n % 4} of {n} elements" in str(e.value)
        sg.inputs_intact()


@pytest.mark.parametrize("name,rows,N,dtype", [("final_conv_blend.out_vid", 15, 24, torch.float32), ("final_conv_blend_u8.frames", 5, 24, torch.uint8),
                                               ("frames_to_yuv420.out", 5, 12, torch.uint8)])
def test_store_one_row_past_a_frame_range_is_rejected(sg, name, rows, N, dtype):
    """Frames [1, 4) of a 5-frame clip (the fp32 clip: of each of its three channels).  The row after the range lies INSIDE the clip: no band
    sees it, the stated rows do; with the range at the end of the clip the same store lands in the back band."""
    per = rows // 5
    for t1, words in ((4, "rows outside the stated written part"), (5, "back band")):
        for defect in (None, "row_past_range"):
            sg.reset()
            clip = sg.guarded_out(rows, N, name=name, dtype=dtype)
            view = clip.view(per, 5, N)[per - 1, 1:t1]                       # the last channel's frames: the row after them is the next frame
            for c in range(per - 1):
                clip.view(per, 5, N)[c, 1:t1] = 1
            sg.fill_frames(view, defect)
            mask = torch.zeros(per, 5, dtype=torch.bool)
            mask[:, 1:t1] = True
            if defect is None:
                sg.verify(written={name: mask.flatten()})
                with pytest.raises(GuardError, match="never written"):       # ... and without the statement the whole clip is due
                    sg.verify()
            else:
                with pytest.raises(GuardError) as e:
                    sg.verify(written={name: mask.flatten()})
                assert str(e.value).startswith(name + ":") and words in str(e.value), str(e.value)


def test_byte_output_with_one_unwritten_byte_is_rejected(sg):
    from guarded import assert_no_255
    x = torch.rand(4, 6, generator=torch.Generator().manual_seed(1)) * 1.2 - 0.1          # clips at both ends; the top level is 254
    want = (x.clamp(0, 1) * 254)[..., None].to(torch.uint8).expand(4, 6, 3)
    assert_no_255(want)
    assert bool((want == 254).any()) and bool((want == 0).any())
    got = sg.to_bytes(sg.guarded_in(x, name="x")[0])
    sg.verify()
    assert torch.equal(got, want)
    sg.reset()
    sg.to_bytes(sg.guarded_in(x, name="x")[0], "one_byte_unwritten")
    with pytest.raises(GuardError, match=r"^to_bytes.out: 1 of 72 elements hold poison.*never written"):
        sg.verify()
    with pytest.raises(AssertionError, match="255 is the poison"):           # expected bytes that reach 255 make the rule ambiguous: refused
        assert_no_255(torch.tensor([0, 255], dtype=torch.uint8))


def test_empty_takes_a_device_where_there_is_no_like_tensor(sg):
    out = sg.empty(3, 2, 4, device="cpu")
    assert out.shape == (3, 2, 4) and out.dtype == torch.float32 and bool(torch.isnan(out).all()) and sg.outs[-1].name.endswith(".out")
    from dawn_pytorch_amd.ops import HipOps
    plain = HipOps.empty(sg, 3, 2, 4, device="cpu")
    assert plain.shape == (3, 2, 4) and plain.dtype == torch.float32
    assert HipOps.empty(sg, (5, 2), like=torch.zeros(1), dtype=torch.uint8).shape == (5, 2)


def test_unnameable_call_site_is_an_error(g):
    like = torch.zeros(1)
    with pytest.raises(GuardError, match="cannot name the buffer"):
        [g.empty(3, like=like)]
    with pytest.raises(GuardError, match=r"head_out.out is in guarded.PARTIAL.*written="):
        g.reset()
        out = g.guarded_out(3, 20, name="head_out.out")
        out[:2] = 1.0
        g.verify()
