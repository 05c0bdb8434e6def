"""The fp32-accuracy gate of tests/split_gate.py on the launches of the LFG flow decoder (flow_decoder.py, csrc/flow_decode.hip, the first
7x7 conv of csrc/misc.hip and the direct split-bf16 3x3 kernel of csrc/conv3x3_split.hip), the stage that produces the pixels.  The gate,
its factor and its floor are split_gate's:

    rel_err(got) <= c * rel_err(base32) + FLOOR,      rel_err(t) = max|t - want64| / max|want64|,      c = C_GATE unless C_WIDE widens it,

want64 = the RefOps op of the case in float64 on the CPU, base32 = the same op in float32 on the CPU (convolutions through torch's
im2col + GEMM: oneDNN and NNPACK off, as split_gate.Case.base32).  tests/test_decode_gate_cpu.py shows on the CPU that every case accepts
base32 and rejects each defect of `Case.defect_names()`, emulated in float64 against the same want64 and checked with the case's own c;
tests/test_hip_decode_fp64_gates.py runs the same cases on the GPU kernels.

kind "dconv"  conv3x3_bf16_v2_kernel at every distinct 3x3 launch of FlowDecoder at the shipped architecture (64 / 128 / 256 channels) for
              256-px and 128-px images.  FlowDecoder hands dawn_conv_gemm only w_bf3, so no Winograd form takes these.  W, C and N are the
              production values (they fix the tile width WT, the column count WN and the chunk count); F and H are reduced: F to the
              fewest frames at the production H, then H to the smallest multiple of the tile height, such that dawn_conv3x3_direct_form
              still answers what it answers at the production shape (DCONV_PROD: 64-frame chunks, 1 frame for the encoder) and the
              image still has three row tiles (top halo, an interior seam, bottom halo).  Defects: drop_third / stale_third on the
              weights, the last 16 input channels of the last tap lost, and the outputs of one interior tile (TR rows x WT columns, the
              second row tile and -- on the column-tiled 128 / 256-pixel-wide levels -- the second 32-column tile) computed from that
              tile's own pixels with its one-pixel halo read as zero.
kind "first"  init_conv_x at the decoder's widths (the MFMA kernel at w = 128: two image rows per tile, w = 256: one) and on the generic
              kernel (w = 40), the bias map as fea_pre as FlowDecoder.encode passes it.  Defects: the weights truncated to 16 mantissa
              bits (the kernel is an fp32 MFMA: what a tf32-class pipe would compute), the last tap lost, and a wrapped patch: the right
              padding of every patch row read from the next image row's first pixels.
kind "warp"   warp_blend on exact-position motion (`dyadic_motion`): displacements in eighths of a latent pixel on power-of-two grids.
              Sampling positions, the x2 / x4 resize weights and the resized flows are then exact in fp32 and in float64, CPU fp32's
              error falls from 1e-6..1e-5 (random grids: the rounding of the position itself) to ~1e-7, and a position error of 1e-4 pixel
              stands far above it.  The defects are emulated in `warp64`, a float64 restatement of the sampler that equals
              RefOps.warp_blend in float64 without them: the position off by 1e-4 pixel, zeros padding replaced by border clamp, the
              resize's upper index not clamped at the last latent row / column (it reads on in memory), the occlusion taken nearest
              instead of bilinear, the ReLU of prev_ab omitted, and with up2 one of the four written pixels taken from the right-hand
              neighbour.  A case lists only the defects that can reach it (no resize: no resize defects ...).
kind "final"  final_conv_blend_kernel, fp32 form (the byte forms are tied to it bit for bit elsewhere).  `conv` cases: conf = 0 and identity
              motion, so out_vid = sigmoid(conv) and no warp noise masks the 49 C-term sum; `blend` cases: dyadic motion at h = H / 4 and
              random conf, both outputs gated.  Defects (on out_vid): the last 8-channel chunk lost, the last tap lost in the last
              channel quad, the first tile's 3-pixel halo towards its neighbours read as zero (multi-tile cases only).  No precision
              defect: the kernel runs on the vector ALUs.
kind "ew"     affine_act and bn_relu_pool2: no defect; the CPU test checks that base32 has a real fp32 error on the data."""
import warnings

import torch
import torch.nn.functional as F_

from oracle.ops_ref import RefOps
from split_gate import (C_GATE, FLOOR, LOG, coherent, drop_third, fp32_gate, gate_rejects, packd, rel_err, stale_third,  # noqa: F401
                        trunc_planes3)

# Gate factors widened past C_GATE: GPU error / CPU fp32 error against float64 measured on an MI355X (max over that kernel's cases), x 1.5,
# rounded up to the next 0.5 (the rule of stage_gate.C_WIDE).  Kernels that are not named here hold C_GATE = 2; their measured maxima:
# init_conv_x_mfma_kernel 1.30 (w = 256; 1.03 at w = 128), init_conv_x_kernel 1.15, warp_blend_kernel 1.49 (16 x 256 from 4 x 64, prev; 0.71 ..
# 1.33 elsewhere), final_conv_blend_kernel 1.73 (one tile, C = 8; 1.55 at C = 64; warped_vid 1.00), affine_act 1.00, bn_relu_pool2 1.00.
C_WIDE = {
    # conv3x3_bf16_v2_kernel at the decoder's launches: one fp32 chain on the matrix pipe over all 9 C products of an output (CPU GEMM blocks
    # its sums), so the ratio grows with K -- a factor per depth, each the rule applied to the cases of that depth, none wider than the
    # one factor (9.0) the deepest would give the whole kernel.  Measured: K = 576 2.46 (down0 at 256 px, eight waves; 2.10 at 128 px);
    # K = 1152 3.47 (up1 at 128 px; 3.35 / 3.06 / 3.03 the others); K = 2304 5.79 (up0 at 256 px, four waves; 5.60 / 5.36 the bottleneck convs
    # on eight waves, 4.54 up0 at 128 px).  test_decode_gate_cpu's weakest defect at each depth (the lost third plane) stands at 11.5, 10.6
    # and 12.3 x CPU fp32.
    "dconv/K576": 4.0,
    "dconv/K1152": 5.5,
    "dconv/K2304": 9.0,
}

HALO, V2_WN1, V2_WN2 = 1, 2, 3          # dawn_conv3x3_direct_form (0: the descriptor does not reach a direct split kernel)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def trunc16(x):
    """x (float32 values) with every element truncated to its top 16 mantissa bits, as float64."""
    p1, p2, _ = trunc_planes3(x.float())
    return p1.double() + p2.double()


def _cpu_fp32(fn):
    """fn() with torch's im2col + GEMM convolution (oneDNN and NNPACK off), as split_gate.Case.base32."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.backends.mkldnn.flags(enabled=False), torch.backends.nnpack.flags(enabled=False):
            return fn()


# ---------------------------------------------------------------------------------------------- exact-position motion
def dyadic_grid64(T, h, w, seed, max_shift):
    """float64 (2, T, h, w) sampling grid and float32 (T, h, w) conf of `dyadic_motion`."""
    assert h & (h - 1) == 0 and w & (w - 1) == 0, "power-of-two latent grids only"
    g = torch.Generator().manual_seed(seed)
    n = int(round(max_shift * 8))
    d = torch.randint(-n, n + 1, (2, T, h, w), generator=g).double() / 8          # latent pixels, in eighths
    d[:, T - 1] *= 3                                                              # the last frame: whole regions sample outside
    xs = torch.arange(w, dtype=torch.float64).view(1, 1, w)
    ys = torch.arange(h, dtype=torch.float64).view(1, h, 1)
    grid = torch.stack(((2 * (xs + d[0]) + 1) / w - 1, (2 * (ys + d[1]) + 1) / h - 1))
    return grid, torch.rand(T, h, w, generator=g)


def dyadic_motion(T, h, w, seed, max_shift):
    """(grid (2, T, h, w), conf (T, h, w)) float32: pixel (y, x) of frame t samples latent position (x + dx, y + dy), dx and dy integers
    over 8 with |d| <= max_shift (x 3 in the last frame): grid = (2 (x + d) + 1) / w - 1 has an integer numerator below 2^24 over the
    power of two 4 w, so it is exact in fp32, and so are the sampling position ((g + 1) W - 1) / 2 at every level and the flows resized
    by 2 and by 4 (weights in eighths).  conf is uniform in [0, 1)."""
    grid, conf = dyadic_grid64(T, h, w, seed, max_shift)
    return grid.float().contiguous(), conf.contiguous()


def identity_motion(T, h, w, conf=None):
    """The grid under which every pixel samples itself (exactly so on power-of-two sizes), and a constant conf plane."""
    gx = ((2 * torch.arange(w, dtype=torch.float64) + 1) / w - 1).view(1, 1, w).expand(T, h, w)
    gy = ((2 * torch.arange(h, dtype=torch.float64) + 1) / h - 1).view(1, h, 1).expand(T, h, w)
    return torch.stack((gx, gy)).float().contiguous(), torch.full((T, h, w), 0.0 if conf is None else conf)


def exact_motions(h, w):
    """[(name, grid (2, T, h, w), expect)] for a same-size level: motions whose warp is known bit for bit.  expect(img (h, w, C)) -> the
    (T, h, w, C) warp of img: identity; whole-pixel shifts (zero fill); positions at exactly -1 and W (H): the one corner inside has
    weight 0; finite far-outside grids."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")

    def grid_of(px, py):                                  # pixel positions (T, h, w) -> the grid that samples them
        return torch.stack(((2 * px + 1) / w - 1, (2 * py + 1) / h - 1)).float().contiguous()

    def shifted(shifts):
        def expect(img):
            out = torch.zeros(len(shifts), h, w, img.shape[2], dtype=img.dtype)
            for t, (dy, dx) in enumerate(shifts):
                y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                out[t, y0:y1, x0:x1] = img[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            return out
        return expect

    def zeros(T):
        return lambda img: torch.zeros(T, h, w, img.shape[2], dtype=img.dtype)
    shifts = ((0, 3), (-2, 0), (5, -7))
    one = torch.ones(1, h, w, dtype=torch.float64)
    far = torch.stack((torch.full((4, h, w), 1e30), torch.full((4, h, w), -1e30)))
    far[0, 1], far[1, 2] = -1e30, 1e30
    far[0, 3], far[1, 3] = grid_of(xs[None], ys[None])[0, 0], 1e30               # x inside, y far outside
    return [("identity", grid_of(xs[None].expand(2, h, w), ys[None].expand(2, h, w)), shifted(((0, 0), (0, 0)))),
            ("whole_pixel", grid_of(torch.stack([xs + dx for _, dx in shifts]), torch.stack([ys + dy for dy, _ in shifts])), shifted(shifts)),
            ("edge_-1_and_W", grid_of(torch.cat((-one, w * one, xs[None], xs[None])), torch.cat((ys[None], ys[None], -one, h * one))), zeros(4)),
            ("far_outside", far.float().contiguous(), zeros(4))]


def exact_warp_cases(h, w, C):
    """[(name, grid, conf, skip (h w, C), want (T h w, C))]: warp_blend in mode `first` on exact_motions, want = warp * conf (one rounding)."""
    skip = rnd(h * w, C, seed=1)
    out = []
    for name, grid, expect in exact_motions(h, w):
        T = grid.shape[1]
        conf = torch.rand(T, h, w, generator=torch.Generator().manual_seed(7)) + 0.25
        out.append((name, grid, conf, skip, (expect(skip.view(h, w, C)) * conf[..., None]).reshape(-1, C)))
    return out


# ---------------------------------------------------------------------------------------------- hooked float64 sampler
# RefOps.warp_blend (F.interpolate bilinear + F.grid_sample bilinear / zeros, align_corners False) restated in float64 with a hook for each
# defect of the module docstring.  Without hooks it is the RefOps op (test_decode_gate_cpu.test_hooked_sampler_is_the_oracle).
def _lerp64(n_out, n_in, unclamped):
    src = ((n_in / n_out) * (torch.arange(n_out, dtype=torch.float64) + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = i0 + 1 if unclamped else i0 + (i0 < n_in - 1).long()
    l1 = src - i0
    return i0, i1, 1 - l1, l1


def _resize64(p, Hs, Ws, unclamped=False, nearest=False):
    """(T, h, w) float64 -> (T, Hs, Ws), bilinear.  unclamped: the upper index runs past the last row / column and reads what follows in
    memory (the next row's first element, the next frame's first row, zero behind the last frame).  nearest: F.interpolate's 'nearest'."""
    T, h, w = p.shape
    if (h, w) == (Hs, Ws):
        return p
    if nearest:
        yi = (torch.arange(Hs, dtype=torch.float64) * (h / Hs)).floor().long()
        xi = (torch.arange(Ws, dtype=torch.float64) * (w / Ws)).floor().long()
        return p[:, yi][:, :, xi]
    y0, y1, ly0, ly1 = (t.view(-1, 1) for t in _lerp64(Hs, h, unclamped))
    x0, x1, lx0, lx1 = (t.view(1, -1) for t in _lerp64(Ws, w, unclamped))
    flat = torch.cat((p.reshape(-1), torch.zeros(h * w + w + 1, dtype=p.dtype)))
    base = (torch.arange(T) * h * w).view(T, 1, 1)

    def at(yi, xi):
        return flat[base + (yi * w + xi)[None]]
    return ly0 * (lx0 * at(y0, x0) + lx1 * at(y0, x1)) + ly1 * (lx0 * at(y1, x0) + lx1 * at(y1, x1))


def _sample64(src, Hs, Ws, gx, gy, shift=0.0, border=False):
    """grid_sample of the (Hs * Ws, C) float64 map at the (T, Hs, Ws) grids.  shift: added to both pixel coordinates; border: indices outside
    the map are clamped to its edge instead of contributing zero."""
    ix = (((gx + 1) * Ws - 1) / 2 + shift).clamp(-2.0, Ws + 1.0)           # (far outside: every corner is outside anyway)
    iy = (((gy + 1) * Hs - 1) / 2 + shift).clamp(-2.0, Hs + 1.0)
    x0, y0 = ix.floor(), iy.floor()
    out = 0
    for yc, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
        for xc, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
            inside = (xc >= 0) & (xc < Ws) & (yc >= 0) & (yc < Hs)
            idx = (yc.clamp(0, Hs - 1) * Ws + xc.clamp(0, Ws - 1)).long()
            wgt = wx * wy if border else wx * wy * inside
            out = out + src[idx] * wgt[..., None]
    return out                                                              # (T, Hs, Ws, C)


DEFECTS_WARP = ("position_1e-4", "border_clamp", "resize_unclamped", "occ_nearest", "no_relu", "up2_neighbour")


def warp64(skip, Hs, Ws, grid, conf, prev=None, prev_ab=None, up2=False, defect=None):
    """RefOps.warp_blend in float64; defect: one of DEFECTS_WARP or None."""
    assert defect is None or defect in DEFECTS_WARP
    T, C = grid.shape[1], skip.shape[1]
    un = defect == "resize_unclamped"
    gx, gy = (_resize64(grid[i].double(), Hs, Ws, unclamped=un) for i in (0, 1))
    oc = _resize64(conf.double(), Hs, Ws, unclamped=un, nearest=defect == "occ_nearest")[..., None]
    out = _sample64(skip.double(), Hs, Ws, gx, gy, shift=1e-4 if defect == "position_1e-4" else 0.0, border=defect == "border_clamp") * oc
    if prev is not None:
        p = prev.double().view(T, Hs, Ws, C)
        if prev_ab is not None:
            p = p * prev_ab[0].double() + prev_ab[1].double()
            if defect != "no_relu":
                p = F_.relu(p)
        out = out + p * (1 - oc)
    if up2:
        big = out.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        if defect == "up2_neighbour":                                       # the fourth written pixel comes from column X + 1
            big[:, 1::2, 1::2] = torch.cat((out[:, :, 1:], out[:, :, -1:]), dim=2)
        out = big
    return out.reshape(-1, C).contiguous()


# ---------------------------------------------------------------------------------------------- cases
def _w7_oihw(w7, Cc):
    """[tap][C / 4][3][4] -> (3, C, 7, 7), as RefOps.final_conv_blend."""
    return w7.view(7, 7, Cc // 4, 3, 4).permute(3, 2, 4, 0, 1).reshape(3, Cc, 7, 7)


class Case:
    """name, kind, parameters.  make() -> the seeded float32 inputs; want64 / base32 -> the two references; defects() -> {name: result of
    the defective op in float64}.  The result of a "final" case is (n, 3, T, H, W): out_vid, then warped_vid for the blend cases."""

    def __init__(self, name, kind, c=None, **p):
        self.name, self.kind, self.p = name, kind, p
        key = f"dconv/K{9 * p['C']}" if kind == "dconv" else kind
        self.c = C_WIDE.get(key, C_GATE) if c is None else c

    def __repr__(self):
        return self.name

    # ------------------------------------------------------------------ inputs
    def make(self):
        p, k = self.p, self.kind
        if k == "dconv":
            F, H, W, C, N = p["F"], p["H"], p["W"], p["C"], p["N"]
            return dict(x=rnd(F * H * W, C, seed=1), w=coherent(rnd(9 * C, N, seed=2, scale=(9 * C) ** -0.5)), bias=rnd(N, seed=3),
                        res=rnd(F * H * W, N, seed=4) if p.get("res") else None)
        if k == "first":
            h, w, Co = p["h"], p["w"], 64
            img = torch.rand(3, 1, h, w, generator=torch.Generator().manual_seed(1))
            bias = rnd(Co, seed=3, scale=0.1)
            return dict(x=img, w3=coherent(rnd(147, Co, seed=2, scale=147 ** -0.5)), fea_pre=bias.view(1, Co).expand(h * w, Co).contiguous())
        if k == "warp":
            T, (Hs, Ws), (h, w), C, mode = 3, p["S"], p["s"], p["C"], p["mode"]
            Ttot, t0 = p.get("view", (T, 0))
            grid, conf = dyadic_motion(Ttot, h, w, seed=Hs + C + len(mode), max_shift=p["shift"])
            return dict(skip=rnd(Hs * Ws, C, seed=1), grid=grid[:, t0:t0 + T], conf=conf[t0:t0 + T].contiguous(),
                        prev=rnd(T * Hs * Ws, C, seed=2) if mode != "first" else None,
                        pa=rnd(C, seed=3) if "ab" in mode else None, pb=rnd(C, seed=4) if "ab" in mode else None)
        if k == "final":
            T, H, W, C = 2, p["H"], p["W"], p["C"]
            if p["form"] == "conv":
                grid, conf = identity_motion(T, H, W)
            else:
                grid, conf = dyadic_motion(T, H // 4, W // 4, seed=H + C, max_shift=1.0)
            return dict(x=rnd(T * H * W, C, seed=1), w7=rnd(49, C // 4, 3, 4, seed=2, scale=(49 * C) ** -0.5), b3=rnd(3, seed=3),
                        src=torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)), grid=grid, conf=conf)
        if k == "ew":
            C = p["C"]
            if p["op"] == "affine":
                wide = rnd(333, p.get("ld", C), seed=1)
                return dict(wide=wide, a=rnd(C, seed=2), b=rnd(C, seed=3))
            return dict(x=rnd(2 * p["H"] * p["W"], C, seed=1), a=rnd(C, seed=2), b=rnd(C, seed=3))
        raise ValueError(k)

    def ew_x(self, wide):
        """The (rows, C) input of an affine_act case: the buffer itself, or columns 32 .. 32 + C of a wider one (strided rows)."""
        C = self.p["C"]
        return wide if wide.shape[1] == C else wide[:, 32:32 + C]

    # ------------------------------------------------------------------ the op
    def ref(self, T_, dtype, **over):
        """The RefOps op on the inputs cast to dtype; `over` replaces inputs (already in dtype)."""
        ops = RefOps()
        k, p = self.kind, self.p
        t = {n: (over[n] if n in over else (v.to(dtype) if torch.is_tensor(v) else v)) for n, v in T_.items()}
        if k == "dconv":
            return ops.conv_gemm(t["x"], packd(t["w"]), p["N"], F=p["F"], Hi=p["H"], Wi=p["W"], KH=3, KW=3, pad=1, bias=t["bias"], res=t["res"])
        if k == "first":
            return ops.init_conv_x(t["x"], t["w3"], t["fea_pre"], 1, p["h"], p["w"], 64)
        if k == "warp":
            return ops.warp_blend(t["skip"], *p["S"], t["grid"], t["conf"], prev=t["prev"], prev_ab=None if t["pa"] is None else (t["pa"], t["pb"]),
                                  up2="up2" in p["mode"])
        if k == "final":
            T, H, W = 2, p["H"], p["W"]
            outs = torch.zeros(2, 3, T, H, W, dtype=dtype)
            ops.final_conv_blend(t["x"], H, W, t["w7"], t["b3"], t["src"], t["grid"], t["conf"], outs[0], outs[1])
            return outs[:len(self.outputs())].contiguous()
        if k == "ew":
            if p["op"] == "affine":
                return ops.affine_act(self.ew_x(t["wide"]), t["a"], t["b"], p["act"]).contiguous()
            return ops.bn_relu_pool2(t["x"], t["a"], t["b"], 2, p["H"], p["W"]).contiguous()
        raise ValueError(k)

    def outputs(self):
        return ("out_vid", "warped_vid") if self.kind == "final" and self.p["form"] == "blend" else ("out",)

    def want64(self, T_):
        return self.ref(T_, torch.float64)

    def base32(self, T_):
        return _cpu_fp32(lambda: self.ref(T_, torch.float32))

    # ------------------------------------------------------------------ geometry
    def tile(self):
        """dconv: (TR rows, WT columns) of a tile of conv3x3_bf16_v2_kernel (256 pixels; 32-column tiles above W = 64)."""
        WT = 32 if self.p["W"] > 64 else self.p["W"]
        return 256 // WT, WT

    def conv_kw(self):
        p = self.p
        return dict(F=p["F"], Hi=p["H"], Wi=p["W"], KH=3, KW=3, stride=1, pad=1)

    # ------------------------------------------------------------------ the defects (see the module docstring)
    def defect_names(self):
        k, p = self.kind, self.p
        if k == "dconv":
            return ("drop_third", "stale_third", "last_chunk_lost", "seam_halo_lost")
        if k == "first":
            return ("trunc16", "last_tap_lost", "wrapped_patch")
        if k == "warp":
            resized, mode = p["S"] != p["s"], p["mode"]
            return (("position_1e-4", "border_clamp") + (("resize_unclamped", "occ_nearest") if resized else ())
                    + (("no_relu",) if "ab" in mode else ()) + (("up2_neighbour",) if "up2" in mode else ()))
        if k == "final":
            return ("last_chunk_lost", "tap_lost") + (("seam_halo_lost",) if p["H"] > 16 or p["W"] > 32 else ())
        return ()

    def defects(self, T_, want64):
        k, p = self.kind, self.p
        out = {}
        if k == "dconv":
            w = T_["w"]
            out["drop_third"] = self.ref(T_, torch.float64, w=drop_third(w))
            out["stale_third"] = self.ref(T_, torch.float64, w=stale_third(w))
            lost = w.double().clone()
            lost[-16:] = 0                                              # k = tap * C + c: the last 16 channels of tap (2, 2)
            out["last_chunk_lost"] = self.ref(T_, torch.float64, w=lost)
            (TR, WT), H, W, C, N = self.tile(), p["H"], p["W"], p["C"], p["N"]
            assert H >= 3 * TR
            c0 = WT if W > WT else 0                                    # frame 0, the second row tile, the second column tile
            own = T_["x"].double().view(p["F"], H, W, C)[0, TR:2 * TR, c0:c0 + WT].permute(2, 0, 1)[None]
            wk = w.double().reshape(3, 3, C, N).permute(3, 2, 0, 1)
            y = F_.conv2d(own, wk, T_["bias"].double(), padding=1)[0].permute(1, 2, 0)
            seam = want64.clone().view(p["F"], H, W, N)
            if T_["res"] is not None:
                y = y + T_["res"].double().view(p["F"], H, W, N)[0, TR:2 * TR, c0:c0 + WT]
            seam[0, TR:2 * TR, c0:c0 + WT] = y
            out["seam_halo_lost"] = seam.view(-1, N)
        elif k == "first":
            w3, h, w = T_["w3"], p["h"], p["w"]
            out["trunc16"] = self.ref(T_, torch.float64, w3=trunc16(w3))
            lost = w3.double().clone()
            lost[-3:] = 0                                               # tap (6, 6), three channels
            out["last_tap_lost"] = self.ref(T_, torch.float64, w3=lost)
            img = T_["x"].double()[:, 0]                                # (3, h, w)
            pad = F_.pad(img, (3, 3, 3, 3))
            pad[:, 3:3 + h - 1, w + 3:] = img[:, 1:, :3]                # right padding of row y = the first pixels of row y + 1
            wk = w3.double().reshape(7, 7, 3, 64).permute(3, 2, 0, 1)
            y = F_.conv2d(pad[None], wk)[0].permute(1, 2, 0).reshape(h * w, 64)
            out["wrapped_patch"] = y + T_["fea_pre"].double()
        elif k == "warp":
            for n in self.defect_names():
                out[n] = self.hooked(T_, n)
        elif k == "final":
            T, H, W, C = 2, p["H"], p["W"], p["C"]
            x, w7, b3 = T_["x"].double(), T_["w7"].double(), T_["b3"].double()

            def sig(x_, w_):
                return torch.sigmoid(F_.conv2d(x_.view(T, H, W, C).permute(0, 3, 1, 2), _w7_oihw(w_, C), b3, padding=3))
            s = sig(x, w7)
            _, occ = RefOps._motion(T_["grid"].double(), T_["conf"].double(), H, W)                     # (T, 1, H, W)

            def with_sigmoid(s_def):                                    # out_vid is linear in the sigmoid: + (s' - s)(1 - occ)
                o = want64.clone()
                o[0] += ((s_def - s) * (1 - occ)).permute(1, 0, 2, 3)
                return o
            xl = x.clone()
            xl[:, -8:] = 0
            out["last_chunk_lost"] = with_sigmoid(sig(xl, w7))
            wl = w7.clone()
            wl[48, -1] = 0
            out["tap_lost"] = with_sigmoid(sig(x, wl))
            if "seam_halo_lost" in self.defect_names():                 # tile (0, 0) = 16 rows x 32 columns, from its own pixels only
                own = torch.zeros_like(x).view(T, H, W, C)
                own[:, :16, :32] = x.view(T, H, W, C)[:, :16, :32]
                sd = s.clone()
                sd[:, :, :16, :32] = sig(own.view(-1, C), w7)[:, :, :16, :32]
                out["seam_halo_lost"] = with_sigmoid(sd)
        assert tuple(out) == self.defect_names(), (self.name, tuple(out))
        return out

    def hooked(self, T_, defect=None):
        """A warp case through warp64."""
        p = self.p
        return warp64(T_["skip"], *p["S"], T_["grid"], T_["conf"], prev=T_["prev"], prev_ab=None if T_["pa"] is None else (T_["pa"], T_["pb"]),
                      up2="up2" in p["mode"], defect=defect)


# ---- dconv: (launch, image size) -> the production shape (F, H, W, C, N, res) and the reduced (F, H) of the rule in the module docstring.
# dawn_conv3x3_direct_form of both is asserted equal, and to DCONV_FORM, by test_decode_gate_cpu (no GPU) and again before every launch.
# The eight-wave tile (V2_WN2) needs (M / 256) * (N / 128) > 128 tiles: 136 rows of 256 pixels at N = 128; at N = 256 more than 16384
# pixels: 5 frames of 52 x 64, 17 frames of 32 x 32.  Everything else runs on four-wave tiles at any size: one frame, three row tiles.
def _dconv_table():
    rows = []
    for px in (256, 128):
        q, h = px // 4, px // 2
        for launch, W, C, N, res, Fp, red, form in (
                ("down0", px, 64, 128, False, 1, (1, 136) if px == 256 else (1, 24), V2_WN2 if px == 256 else V2_WN1),
                ("down1", h, 128, 256, False, 1, (1, 24) if h == 128 else (1, 12), V2_WN1),
                ("bott_conv1", q, 256, 256, False, 64, (5, 52) if q == 64 else (17, 32), V2_WN2),
                ("bott_conv2_res", q, 256, 256, True, 64, (5, 52) if q == 64 else (17, 32), V2_WN2),
                ("up0", h, 256, 128, False, 64, (1, 24) if h == 128 else (1, 12), V2_WN1),
                ("up1", px, 128, 64, False, 64, (1, 24), V2_WN1)):
            rows.append((f"{launch}_{px}px", dict(F=Fp, H=W, W=W, C=C, N=N, res=res), red, form))
    return rows


DCONV = _dconv_table()
DCONV_PROD = {f"dconv/{n}": prod for n, prod, _, _ in DCONV}
DCONV_FORM = {f"dconv/{n}": form for n, _, _, form in DCONV}

WARP_SIZES = (((16, 32), (16, 32), 3.0), ((32, 64), (16, 32), 3.0), ((64, 128), (16, 32), 3.0), ((16, 256), (4, 64), 1.0))   # (Hs, Ws), (h, w), max shift
WARP_MODES = ("first", "prev", "prev_ab", "prev_ab_up2", "prev_up2")
WARP_C = (4, 8, 64)

CASES = [
    *[Case(f"dconv/{n}", "dconv", **dict(prod, F=red[0], H=red[1])) for n, prod, red, _ in DCONV],
    Case("first/mfma_8x128", "first", h=8, w=128),
    Case("first/mfma_8x256", "first", h=8, w=256),
    Case("first/generic_8x40", "first", h=8, w=40),
    # every size x mode, the channel count cycling so that each size and each mode meets 4, 8 and 64 channels
    *[Case(f"warp/{S[0]}x{S[1]}_from_{s[0]}x{s[1]}_C{WARP_C[(i + j) % 3]}_{m}", "warp", S=S, s=s, shift=sh, C=WARP_C[(i + j) % 3], mode=m)
      for i, (S, s, sh) in enumerate(WARP_SIZES) for j, m in enumerate(WARP_MODES)],
    # frames [2, 5) of a 7-frame clip: the grid's plane stride is 7 h w, not T h w
    Case("warp/32x64_from_16x32_C8_prev_ab_view2of7", "warp", S=(32, 64), s=(16, 32), shift=3.0, C=8, mode="prev_ab", view=(7, 2)),
    Case("final/conv_16x32_C8", "final", form="conv", H=16, W=32, C=8),             # exactly one tile, one chunk
    Case("final/conv_17x33_C24", "final", form="conv", H=17, W=33, C=24),           # four tiles, three of them one pixel wide or high
    Case("final/conv_8x8_C16", "final", form="conv", H=8, W=8, C=16),               # a lone partial tile
    Case("final/conv_32x64_C64", "final", form="conv", H=32, W=64, C=64),           # four full tiles at the shipped C
    Case("final/blend_16x32_C8", "final", form="blend", H=16, W=32, C=8),
    Case("final/blend_32x64_C64", "final", form="blend", H=32, W=64, C=64),
    Case("ew/affine_C4_relu", "ew", op="affine", C=4, act=1),
    Case("ew/affine_C96_none", "ew", op="affine", C=96, act=0),
    Case("ew/affine_C96_relu_strided", "ew", op="affine", C=96, act=1, ld=160),
    Case("ew/bn_relu_pool2_2x2", "ew", op="pool", C=48, H=2, W=2),
    Case("ew/bn_relu_pool2_12x20", "ew", op="pool", C=48, H=12, W=20),
]
