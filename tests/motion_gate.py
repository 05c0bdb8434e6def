"""The fp32-accuracy gate of tests/split_gate.py on the five kernels of the LFG motion encode (csrc/motion_encode.hip), off the shapes of the
stage goldens: non-square maps, ragged last workgroups, R = 1 and R = 15, every antialias scale, the production width of bg_params, and
motion parameters built to reach the branches a random tiny model does not.  The gate, its factor and its floor are split_gate's:

    rel_err(got) <= c * rel_err(base32) + FLOOR,      rel_err(t) = max|t - want64| / max|want64|,      c = C_GATE unless C_WIDE widens it,

want64 = the restatement of tests/motion_cases.py in float64 (pinned to the reference's stage outputs by tests/test_motion_cpu.py), base32
= the same restatement in float32 on the CPU; the coordinate grid is the fp32 grid in both (an input).  tests/test_motion_gate_cpu.py shows
on the CPU that every case accepts base32 and rejects each defect of `Case.defect_names()`, emulated in float64 against the same want64
and checked with the case's own c; tests/test_hip_motion_fp64_gates.py runs the same cases on the GPU kernels.

kind "aa"  dawn_antialias_down.  Bytes from an integer formula and the same frames as fp32 planes (byte / 255); sizes that are no multiple
           of s, partial tiles, two tile rows, s = 8 (K = 29, AA_MAX_ROWS LDS rows), s = 2, s = 3, s = 1 (exact).  Defects: replicate for
           zero padding, the last tap of the vertical pass lost, the kept pixel at s o + 1, a second tile row that reads the input rows
           above its first kept row as zero (a lost LDS halo; cases with more than 16 output rows), bytes / 256.
kind "rm"  dawn_region_moments on anisotropic log-Gaussian bumps times the temperature: centres off the grid centre (RM_RADIUS), rotated
           covariances, every region's relative eigen-gap >= RM_GAP_FLOOR, rows 16 wide with NaN past R.  Gated: shift, covar; affine
           against sqrt_factor(covar64) at the project tolerance over the eigen-gap.  Defects: x normalised by h - 1 and y by w - 1, the
           pixels past the last whole 256-stride lost, wave 1's partial sums lost, the covariance as E[gg] - mean^2 from float32 sums.
kind "bg"  dawn_bg_params up to C = 1024 (every thread four channels, all four waves), npix 144 .. 1, ld > C with NaN behind C.  Defects:
           channels >= 256 lost, the channels of waves 1-3 lost, the mean over npix - 1, and at npix = 144 sequential float32 spatial sums.
kind "mi"  dawn_motion_inputs and kind "fc" dawn_flow_combine on shared parameter sets (`motion_params`), two families:
           exact   -- sides 2^k + 1 (the fp32 grid and the pixel position ((g + 1) W - 1) / 2 are exact), A_s and A_d diagonal or
                      quarter-turned with power-of-two entries, so that M = A_s inverse(A_d) is a signed power-of-two matrix, shifts in
                      64ths: every region's sparse motion and sampling position is the same number in fp32 and in float64, CPU fp32 stays
                      below EXACT_BASE32_MAX, and a position off by 1e-4 pixel stands three orders above it;
           random  -- seeded parameters, as production would give.
           Both carry, in the last frame (R = 1 has one region: T = 4 and one of the three in each of the frames 1 .. 3): a region with
           M[0][0] < 0 before the sign fix, a region with M[0][0] == 0 exactly (a quarter turn: M is zeroed, as torch.sign does), a region
           that samples wholly outside, and a bg whose third row is (a, b, 1) with |a|, |b| <= 0.1.  Defects of mi: the axis swap, the
           position off by 1e-4 pixel, border clamp for zeros, the sign fix omitted, sign(0) taken as 1, the background motion not
           divided by Z, the heatmap from the covariance instead of its inverse, the last hw % 64 pixels left zero.  Defects of fc: the
           axis swap, the softmax over R masks, the occlusion read from channel R, the background term not divided by Z, the sign fix
           omitted.  `mi64` / `fc64` restate both ops in float64 with a hook per defect; without one they equal motion_cases'.
A case lists only the defects that can reach it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import motion_cases as mc
from decode_gate import _sample64
from split_gate import C_GATE, FLOOR, fp32_gate, gate_rejects, rel_err  # noqa: F401

# Gate factors widened past C_GATE: GPU error / CPU fp32 error against float64 measured on an MI355X (max over that kernel's cases), x 1.5,
# rounded up to the next 0.5 (the rule of stage_gate.C_WIDE), keyed "kind/output".  profiles/motion_gate_ratios.md has every kernel's
# measured maximum; the outputs that are not named here hold C_GATE = 2.
C_WIDE = {}

TEMPERATURE = mc.TEMPERATURE
EXACT_BASE32_MAX = 5e-7          # CPU fp32 on the exact family: a condition on the inputs (test_motion_gate_cpu asserts it)
RM_GAP_FLOOR = 0.05              # relative eigen-gap of every region of every rm case
RM_RADIUS = 1.0                  # |centre| of the rm bumps: on the border.  The E[gg] - mean^2 defect loses ~ mean^2 / covar ulps of the
#                                  covariance.  Its error over its bound (2 x CPU fp32 + 1e-7), weakest of the four cases: 0.40 at radius
#                                  0.3, 1.37 at 0.55, 2.57 at 0.8, 4.28 at 1.0 (5.72, 8.97, 4.28, 4.55 in the order of RM_SHAPES)
LD_ROWS = 16


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def gate_frames_u8(T, H, W):
    """(T,H,W,3) uint8: motion_cases.frames_u8's triangle waves of drifting quadratic forms, at any size."""
    y = np.arange(H, dtype=np.int64).reshape(1, H, 1, 1)
    x = np.arange(W, dtype=np.int64).reshape(1, 1, W, 1)
    ch = np.arange(3, dtype=np.int64).reshape(1, 1, 1, 3)
    t = np.arange(T, dtype=np.int64).reshape(T, 1, 1, 1)
    q = ((y - H // 2 - 3 * t) ** 2 * (ch + 2) + (x - W // 3 - 5 * t) ** 2 * (4 - ch) + (x * y * (t + 2)) // 3) * 2040 // (H * W) + 61 * ch + 17 * t
    return torch.from_numpy(np.abs(q % 510 - 255).astype(np.uint8))


def pad16(n):
    return -(-n // 16) * 16


def wide_rows(x, ld):
    """x (rows, C) inside a (rows, ld) buffer whose other columns hold NaN."""
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = x
    return buf


# ---------------------------------------------------------------------------------------------- antialias_down, float64 with hooks
def aa64(x, s, replicate=False, lose_last_vtap=False, offset=0):
    """motion_cases.antialias_down in float64; replicate: the padding repeats the border pixel; lose_last_vtap: the kernel's last row
    (the last tap of the vertical pass) contributes nothing, the divisor stays; offset: the kept pixel is s o + offset."""
    H, W = x.shape[2:]
    k2 = mc.aa_kernel(s).double().clone()
    ka = k2.shape[0] // 2
    if lose_last_vtap:
        k2[-1, :] = 0
    xp = F.pad(x.double(), (ka, ka + offset, ka, ka + offset), mode="replicate" if replicate else "constant")
    out = F.conv2d(xp, k2.view(1, 1, *k2.shape).repeat(3, 1, 1, 1), groups=3)
    return out[:, :, offset::s, offset::s][:, :, :-(-H // s), :-(-W // s)]


def aa_running_sum_divisor(s):
    """(the divisor as a running float32 sum of the K x K float32 products, row by row; the same sum in float64): what the host of
    dawn_antialias_down once divided by, and what it divides by now (rounded once)."""
    g = mc.aa_kernel(s) if s == 1 else torch.exp(-(torch.arange(4 * (s - 1) + 1, dtype=torch.float32) - 2 * (s - 1)) ** 2 / (2 * ((s - 1) / 2) ** 2))
    prod = (g.view(-1, 1) * g.view(1, -1)).reshape(-1)
    run = torch.zeros((), dtype=torch.float32)
    for v in prod:
        run = run + v
    return float(run), float(prod.double().sum())


def aa_format_bound(s):
    """A bound on rel_err of dawn_antialias_down against float64 from the number format alone, for non-negative frames.  An output is two
    chains of K fused multiply-adds of non-negative terms, one division, and a divisor rounded once: 2 K + 2 roundings, each at most
    u = 2^-24 of a partial sum that never exceeds the final one, of either sign.  Their sum is a random walk of standard deviation
    <= 0.29 u sqrt(2 K + 2); 2 u sqrt(2 K) + 3 u is seven of those (the 3 u: the division, the divisor, and the reference's own fp32
    divisor, which want64 shares).  At s = 8 (K = 29) that is 1.1e-6: the kernel stands at 2.2e-7, a running-sum divisor at 2.9e-6 --
    where the fp32 gate cannot tell them apart, because CPU fp32's own 841-tap convolution is at 1.4e-6."""
    K = 4 * (s - 1) + 1
    return (2 * math.sqrt(2 * K) + 3) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------- region_moments
def rm_inputs(T, h, w, R, radius=RM_RADIUS, isotropic=False):
    """x (T, h*w, R) float32 = temperature * log of an anisotropic Gaussian per (frame, region): softmax(x / temperature) is that Gaussian
    on the grid.  Centres on a circle of `radius` around the grid centre, moving with the frame; axes sigma and 0.55 sigma, rotated."""
    g = mc.coordinate_grid(h, w).reshape(h * w, 2)
    x = torch.empty(T, h * w, R, dtype=torch.float64)
    for t in range(T):
        for r in range(R):
            phi = 2 * math.pi * r / R + 0.7 * t + 0.3
            th = 0.4 + 1.1 * r + 0.5 * t
            s1 = 0.30 + 0.02 * (r % 5)
            s2 = s1 if isotropic else 0.55 * s1
            c = torch.tensor([0.0, 0.0] if isotropic else [(radius + 0.03 * t) * math.cos(phi), (radius + 0.03 * t) * math.sin(phi)], dtype=torch.float64)
            rot = torch.tensor([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]], dtype=torch.float64)
            ci = rot @ torch.diag(torch.tensor([s1 ** -2, s2 ** -2], dtype=torch.float64)) @ rot.t()
            d = g - c
            x[t, :, r] = -0.5 * torch.einsum("pa,ab,pb->p", d, ci, d) * TEMPERATURE
    return x.float()


def moments64(x, g, keep=None, temperature=TEMPERATURE):
    """shift and covar of motion_cases.region_moments in float64 on the grid g (h*w, 2); keep (h*w,) bool: the other pixels are lost."""
    z = x.double() / temperature
    if keep is not None:
        z = z.masked_fill(~keep.view(1, -1, 1), float("-inf"))
    p = torch.softmax(z, dim=1)
    shift = torch.einsum("tpr,pc->trc", p, g)
    d = g.view(1, 1, -1, 2) - shift.unsqueeze(2)
    return dict(shift=shift, covar=torch.einsum("tpr,trpa,trpb->trab", p, d, d))


def moments_f32_sums(x, h, w, temperature=TEMPERATURE):
    """The one-pass form entirely in float32: S, S g, S g g^T as float32 sums, covar = E[g g^T] - mean mean^T."""
    xf = x.float()
    e = torch.exp((xf - xf.amax(dim=1, keepdim=True)) / temperature)
    g = mc.coordinate_grid(h, w, torch.float32).reshape(h * w, 2)
    S = e.sum(dim=1)
    m = torch.einsum("tpr,pc->trc", e, g) / S.unsqueeze(-1)
    gg = torch.einsum("tpr,pa,pb->trab", e, g, g) / S.view(*S.shape, 1, 1)
    return dict(shift=m.double(), covar=(gg - m.unsqueeze(-1) * m.unsqueeze(-2)).double())


def affine_bound(covar64):
    """Per region: (sqrt_factor(covar64), the project tolerance 1e-4 max(1, |A|) over the relative eigen-gap) -- check_motion_matrices' bound."""
    a64 = mc.sqrt_factor(covar64)
    return a64, 1e-4 * a64.abs().amax(dim=(-1, -2)).clamp(min=1.0) / mc.eigen_gap(covar64)


def check_affine(aff, covar64, what):
    """affine against sqrt_factor(covar64) at the eigen-gap bound, A A^T = covar64 at the project tolerance, det(affine) < 0."""
    aff = aff.detach().cpu().double()
    a64, bound = affine_bound(covar64)
    err = (aff - a64).abs().amax(dim=(-1, -2))
    print(f"{what}: max |A - A64| {float(err.max()):.3g}, worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all()), (what, float((err / bound).max()))
    mc.assert_close(aff @ aff.transpose(-1, -2), covar64, what + ": A A^T = covar")
    assert bool((torch.det(aff) < 0).all()), what


# ---------------------------------------------------------------------------------------------- bg_params
def bg_activations(T, npix, C):
    """(T, npix, C) float32, ReLU-like: a per-channel floor off_c in [1.5, 1.9] plus relu(noise - 1), so ~84 % of a channel's pixels sit
    exactly on its floor.  The floor's bits below 2^-16 are 2^-17 - 2^-23: a running float32 sum that has passed 128 (one ulp = 2^-16
    there; at npix = 144 it does after ~75 pixels) loses ~2^-17 with every floor pixel it adds, always downwards, in every channel -- a
    bias that fc's signed weights cannot average away.  On unstructured activations sequential float32 sums over 144 pixels err by
    ~2e-7, no more than CPU fp32's own mean and GEMV, and no gate factor tells the two apart (measured: 0.36 .. 0.51 x the bound; on these activations the defect stands at 4.26 x)."""
    g = torch.Generator().manual_seed(5)
    off = (torch.floor((1.5 + 0.4 * torch.rand(C, generator=g).double()) * 2 ** 16) / 2 ** 16 + 2.0 ** -17 - 2.0 ** -23).float()
    return off + torch.relu(rnd(T, npix, C, seed=1) - 1.0)


def bg64(x, fc_w, fc_b, keep=None, div=None, f32_sums=False):
    """motion_cases.bg_params in float64 on x (T, npix, C); keep (C,) bool: the other channels are lost; div: the mean's divisor;
    f32_sums: the spatial sum of each channel runs in float32, pixel after pixel."""
    T, npix, _ = x.shape
    if f32_sums:
        s = torch.zeros(T, x.shape[2], dtype=torch.float32)
        for p in range(npix):
            s = s + x[:, p].float()
        s = s.double()
    else:
        s = x.double().sum(dim=1)
    mean = s / (npix if div is None else div)
    if keep is not None:
        mean = mean * keep.double()
    out = torch.eye(3, dtype=torch.float64).repeat(T, 1, 1)
    out[:, :2, :] = (mean @ fc_w.double().t() + fc_b.double()).view(T, 2, 3)
    return out


# ---------------------------------------------------------------------------------------------- motion parameters
def special_slots(R):
    """-> (T, {what: (frame, region)}) for what in neg, zero, outside: the last frame's regions 0, 1, 2; with fewer than three regions one
    of them in each of the last three frames of a longer clip."""
    if R >= 3:
        return 2, dict(neg=(1, 0), zero=(1, 1), outside=(1, 2))
    return 4, dict(neg=(1, 0), zero=(2, 0), outside=(3, 0))


def _diag(a, d):
    return torch.tensor([[a, 0.0], [0.0, d]], dtype=torch.float64)


QUARTER = torch.tensor([[0.0, -1.0], [1.0, 0.0]], dtype=torch.float64)
OUT_SHIFT = torch.tensor([-5.5, 5.25], dtype=torch.float64)      # the driving shift of the region that samples outside: k = g / 2 -+ 2.7 + shift_s


def motion_params(family, h, w, R, seed):
    """-> dict(T, drv = (shift (T,R,2), covar (T,R,2,2), affine (T,R,2,2)), src = the same without T, bg (T,3,3), slots), float32.
    covar = affine affine^T.  See the module docstring for the two families and the special regions."""
    T, slots = special_slots(R)
    g = torch.Generator().manual_seed(seed)
    zr = slots["zero"][1]
    if family == "exact":
        # A_s diagonal with power-of-two entries (det < 0), A_d = A_s inverse(D): M = D, one of six signed power-of-two diagonals
        Ds = [_diag(1, 1), _diag(2, 2), _diag(0.5, 0.5), _diag(1, -1), _diag(2, -2), _diag(0.5, -0.5)]
        As = torch.stack([_diag(2.0 ** -(1 + r % 3), -2.0 ** -(1 + (r // 3) % 2)) for r in range(R)])
        Ad = torch.stack([torch.stack([As[r] @ torch.inverse(Ds[(r + 2 * t) % 6]) for r in range(R)]) for t in range(T)])
        s_shift = torch.randint(-32, 33, (R, 2), generator=g).double() / 64
        d_shift = torch.randint(-32, 33, (T, R, 2), generator=g).double() / 64
        bg = torch.eye(3, dtype=torch.float64).repeat(T, 1, 1)
        bg[:, :2, 2] = torch.randint(-16, 17, (T, 2), generator=g).double() / 64
        # the last frame: Z = 1 + gx / 16 - gy / 32 and (X, Y) = (Z / 4, -Z / 2), all exact, so the background samples the one point
        # (1/4, -1/2) -- a quotient that varies with the pixel has a full mantissa, and the + 1 of the pixel position then rounds by up to
        # 6e-8 W / 2 pixel (measured: CPU fp32 at 1.4e-6 on 17 x 33); the random family has such a bg
        third = torch.tensor([0.0625, -0.03125, 1.0], dtype=torch.float64)
        bg[T - 1] = torch.stack((0.25 * third, -0.5 * third, third))
    else:
        th = torch.rand(T + 1, R, generator=g) * 2 * math.pi
        s1 = 0.15 + 0.25 * torch.rand(T + 1, R, generator=g)
        s2 = 0.15 + 0.25 * torch.rand(T + 1, R, generator=g)
        rot = torch.stack((torch.stack((th.cos(), -th.sin()), -1), torch.stack((th.sin(), th.cos()), -1)), -2).double()
        A = rot @ torch.diag_embed(torch.stack((s1, -s2), -1)).double()
        As, Ad = A[0], A[1:]
        s_shift = (torch.randn(R, 2, generator=g) * 0.25).double()
        d_shift = (torch.randn(T, R, 2, generator=g) * 0.25).double()
        bg = torch.eye(3, dtype=torch.float64).repeat(T, 1, 1)
        bg[:, :2, :] += torch.randn(T, 2, 3, generator=g).double() * 0.05
        bg[T - 1, 2, :2] = torch.tensor([0.08, -0.06], dtype=torch.float64)
    As, Ad = As.clone(), Ad.clone()
    # M[0][0] == 0 exactly: the source's matrix is a quarter turn of a power-of-two diagonal; the driving one is that diagonal in the
    # slot's frame and another quarter-turned diagonal in the others (M is then a positive diagonal there)
    As[zr] = QUARTER @ _diag(0.25, -0.5)
    for t in range(T):
        Ad[t, zr] = _diag(0.5, -0.25) if t == slots["zero"][0] else QUARTER @ _diag(0.5, -0.5)
    t, r = slots["neg"]
    if r == zr:
        Ad[t, r] = As[r] @ _diag(2, -2)              # the quarter turn swaps the diagonal: M = diag(-1/2, 1/2)
    else:
        Ad[t, r] = As[r] @ _diag(-2, 2) if family == "exact" else -1.25 * As[r]               # M = diag(-1/2, 1/2), M = -0.8 I
    t, r = slots["outside"]
    Ad[t, r] = 2 * As[r]                                                                      # M = I / 2
    d_shift[t, r] = OUT_SHIFT
    f = lambda v: v.float().contiguous()                                                      # noqa: E731
    return dict(T=T, slots=slots, drv=(f(d_shift), f(Ad @ Ad.transpose(-1, -2)), f(Ad)), src=(f(s_shift), f(As @ As.transpose(-1, -2)), f(As)),
                bg=f(bg))


# ---------------------------------------------------------------------------------------------- motion_inputs / flow_combine, float64 with hooks
DEFECTS_MI = ("axis_swap", "position_1e-4", "border_clamp", "no_sign_fix", "sign0_is_1", "bg_no_Z", "heat_from_covar", "tail_zero")
DEFECTS_FC = ("axis_swap", "softmax_R", "occ_channel_R", "bg_no_Z", "no_sign_fix")


def grid64(h, w, swap=False):
    """The fp32 coordinate grid as float64; swap: x normalised by h - 1 and y by w - 1."""
    if not swap:
        return mc.coordinate_grid(h, w)
    x = 2 * (torch.arange(w).float() / (h - 1)) - 1
    y = 2 * (torch.arange(h).float() / (w - 1)) - 1
    return torch.stack((x.view(1, w).expand(h, w), y.view(h, 1).expand(h, w)), 2).double()


def motions64(drv, src, bg, h, w, defect=None):
    """motion_cases.sparse_motions in float64, (T, R+1, h, w, 2), with the hooks axis_swap, no_sign_fix, sign0_is_1, bg_no_Z."""
    g = grid64(h, w, swap=defect == "axis_swap")
    T = drv[0].shape[0]
    M = src[2].double().unsqueeze(0) @ torch.inverse(drv[2].double())
    sg = torch.sign(M[..., 0:1, 0:1])
    if defect == "no_sign_fix":
        sg = torch.ones_like(sg)
    elif defect == "sign0_is_1":
        sg = torch.where(sg == 0, torch.ones_like(sg), sg)
    M = M * sg
    d = g.view(1, 1, h, w, 2) - drv[0].double().view(T, -1, 1, 1, 2)
    k = torch.einsum("trab,trhwb->trhwa", M, d) + src[0].double().view(1, -1, 1, 1, 2)
    gh = torch.cat((g, torch.ones(h, w, 1, dtype=torch.float64)), 2)
    b = torch.einsum("tab,hwb->thwa", bg.double(), gh)
    b = b[..., :2] if defect == "bg_no_Z" else b[..., :2] / b[..., 2:3]
    return torch.cat((b.unsqueeze(1), k), 1)


def mi64(drv, src, bg, src_down, defect=None):
    """motion_cases.motion_inputs in float64, (T, 4 (R+1), h, w); defect: one of DEFECTS_MI or None."""
    assert defect is None or defect in DEFECTS_MI
    _, h, w = src_down.shape
    T = drv[0].shape[0]
    g = grid64(h, w, swap=defect == "axis_swap")

    def gauss(shift, covar):
        d = g - shift.double().unsqueeze(-2).unsqueeze(-2)
        ci = covar.double() if defect == "heat_from_covar" else torch.inverse(covar.double())
        return torch.exp(-0.5 * torch.einsum("...hwa,...ab,...hwb->...hw", d, ci, d))
    heat = gauss(drv[0], drv[1]) - gauss(src[0], src[1]).unsqueeze(0)
    heat = torch.cat((torch.zeros(T, 1, h, w, dtype=torch.float64), heat), 1)
    m = motions64(drv, src, bg, h, w, defect)
    K = m.shape[1]
    mm = m.reshape(T * K, h, w, 2)
    warped = _sample64(src_down.double().reshape(3, h * w).t(), h, w, mm[..., 0], mm[..., 1], shift=1e-4 if defect == "position_1e-4" else 0.0,
                       border=defect == "border_clamp").view(T, K, h, w, 3).permute(0, 1, 4, 2, 3)
    out = torch.cat((heat.unsqueeze(2), warped), 2).reshape(T, K * 4, h * w).clone()
    if defect == "tail_zero":
        out[:, :, (h * w) // 64 * 64:] = 0
    return out.view(T, K * 4, h, w)


def fc64(x, drv, src, bg, defect=None):
    """motion_cases.flow_combine in float64: (flow (T,h,w,2), occlusion (T,1,h,w)); defect: one of DEFECTS_FC or None."""
    assert defect is None or defect in DEFECTS_FC
    T, C, h, w = x.shape
    R = C - 2
    m = motions64(drv, src, bg, h, w, defect)
    n = R if defect == "softmax_R" else R + 1
    mask = torch.softmax(x[:, :n].double(), dim=1)
    occ = torch.sigmoid(x[:, R:R + 1].double() if defect == "occ_channel_R" else x[:, R + 1:].double())
    return (m[:, :n] * mask.unsqueeze(-1)).sum(dim=1), occ


def split_mi(maps):
    """(T, 4 K, h, w) -> dict(heat (T,K,h,w), warped (T,K,3,h,w))."""
    T, C, h, w = maps.shape
    v = maps.reshape(T, C // 4, 4, h, w)
    return dict(heat=v[:, :, 0], warped=v[:, :, 1:])


def outside_share(drv, src, bg, h, w):
    """The share of (frame, motion, pixel) samples whose four corners all lie outside the source."""
    m = motions64(drv, src, bg, h, w)
    ix, iy = ((m[..., 0] + 1) * w - 1) / 2, ((m[..., 1] + 1) * h - 1) / 2
    return float(((ix <= -1) | (ix >= w) | (iy <= -1) | (iy >= h)).double().mean())


# ---------------------------------------------------------------------------------------------- cases
class Case:
    """name, kind, parameters.  make() -> the seeded inputs; want64 / base32 -> {output: tensor}, the two references; gated() -> the outputs
    under fp32_gate; defects() -> {name: {output: tensor}}, the defective op in float64."""

    def __init__(self, name, kind, **p):
        self.name, self.kind, self.p = name, kind, p

    def __repr__(self):
        return self.name

    def c(self, out):
        return C_WIDE.get(f"{self.kind}/{out}", C_GATE)

    def gated(self):
        return {"aa": ("out",), "rm": ("shift", "covar"), "bg": ("out",), "mi": ("heat", "warped"), "fc": ("flow", "occ", "occ_x0")}[self.kind]

    # ------------------------------------------------------------------ inputs
    def make(self):
        p, k = self.p, self.kind
        if k == "aa":
            u8 = gate_frames_u8(2, p["H"], p["W"])
            return dict(u8=u8, x=mc.to_float(u8.numpy()))
        if k == "rm":
            x = rm_inputs(2, p["h"], p["w"], p["R"])
            return dict(x=x, rows=wide_rows(x.reshape(-1, p["R"]), LD_ROWS))
        if k == "bg":
            C, npix, ld = p["C"], p["npix"], p["ld"]
            x = bg_activations(2, npix, C)
            return dict(x=x, rows=wide_rows(x.reshape(-1, C), ld), fc_w=rnd(6, C, seed=2, scale=C ** -0.5), fc_b=rnd(6, seed=3, scale=0.1))
        if k in ("mi", "fc"):
            h, w, R = p["h"], p["w"], p["R"]
            P = motion_params(p["family"], h, w, R, seed=7 * h + R)
            if k == "mi":
                src_down = torch.rand(3, h, w, generator=torch.Generator().manual_seed(11))
                P.update(src_down=src_down, src_rows=wide_rows(src_down.reshape(3, h * w).t(), LD_ROWS))
            else:
                x = rnd(P["T"], R + 2, h, w, seed=13, scale=2.0)
                P.update(x=x, rows=wide_rows(mc.rows_of(x), pad16(R + 2)))
            return P
        raise ValueError(k)

    # ------------------------------------------------------------------ the op
    def ref(self, T_, dtype):
        p, k = self.p, self.kind
        if k == "aa":
            return dict(out=mc.antialias_down(T_["x"], p["s"], dtype=dtype))
        if k == "rm":
            shift, covar, affine = mc.region_moments(T_["x"], p["h"], p["w"], TEMPERATURE, dtype=dtype)
            return dict(shift=shift, covar=covar, affine=affine)
        if k == "bg":
            return dict(out=mc.bg_params(T_["x"], T_["fc_w"], T_["fc_b"], dtype=dtype))
        if k == "mi":
            return split_mi(mc.motion_inputs(T_["drv"], T_["src"], T_["bg"], T_["src_down"], dtype=dtype))
        if k == "fc":
            flow, occ = mc.flow_combine(T_["x"], T_["drv"], T_["src"], T_["bg"], dtype=dtype)
            return dict(flow=flow, occ=occ, occ_x0=2 * occ - 1)
        raise ValueError(k)

    def want64(self, T_):
        return self.ref(T_, torch.float64)

    def base32(self, T_):
        return self.ref(T_, torch.float32)

    # ------------------------------------------------------------------ the defects (see the module docstring)
    def out_hw(self):
        p = self.p
        return -(-p["H"] // p["s"]), -(-p["W"] // p["s"])

    def defect_names(self):
        p, k = self.p, self.kind
        if k == "aa":
            if p["s"] == 1:
                return ("kept_plus_1", "bytes_256")
            return ("replicate_pad", "last_vtap_lost", "kept_plus_1") + (("halo_lost",) if self.out_hw()[0] > 16 else ()) + ("bytes_256",)
        if k == "rm":
            hw = p["h"] * p["w"]
            return ("axis_swap",) + (("tail_lost",) if hw > 256 and hw % 256 else ()) + (("wave_lost",) if hw > 64 else ()) + ("f32_one_pass",)
        if k == "bg":
            C, npix = p["C"], p["npix"]
            return ((("channels_256_lost",) if C > 256 else ()) + (("waves_1_3_lost",) if C > 64 else ()) + (("mean_npix_1",) if npix > 1 else ())
                    + (("f32_sums",) if npix == 144 else ()))
        hw = p["h"] * p["w"]
        if k == "mi":
            return tuple(d for d in DEFECTS_MI if (d != "tail_zero" or hw % 64) and (d != "axis_swap" or p["h"] != p["w"]))
        return tuple(d for d in DEFECTS_FC if d != "axis_swap" or p["h"] != p["w"])

    def defects(self, T_, want64):
        p, k = self.p, self.kind
        out = {}
        if k == "aa":
            x, s = T_["x"], p["s"]
            for n in self.defect_names():
                if n == "halo_lost":                     # the second tile row: outputs 16 .., whose tile's first kept row is s * 16
                    cut = x.double().clone()
                    cut[:, :, :s * 16] = 0
                    y = want64["out"].clone()
                    y[:, :, 16:] = aa64(cut, s)[:, :, 16:]
                else:
                    y = {"replicate_pad": lambda: aa64(x, s, replicate=True), "last_vtap_lost": lambda: aa64(x, s, lose_last_vtap=True),
                         "kept_plus_1": lambda: aa64(x, s, offset=1), "bytes_256": lambda: aa64(T_["u8"].permute(0, 3, 1, 2).double() / 256, s)}[n]()
                out[n] = dict(out=y)
        elif k == "rm":
            h, w = p["h"], p["w"]
            pix = torch.arange(h * w)
            g = grid64(h, w).reshape(h * w, 2)
            for n in self.defect_names():
                out[n] = {"axis_swap": lambda: moments64(T_["x"], grid64(h, w, swap=True).reshape(h * w, 2)),
                          "tail_lost": lambda: moments64(T_["x"], g, keep=pix < (h * w) // 256 * 256),
                          "wave_lost": lambda: moments64(T_["x"], g, keep=(pix % 256) // 64 != 1),
                          "f32_one_pass": lambda: moments_f32_sums(T_["x"], h, w)}[n]()
        elif k == "bg":
            ch = torch.arange(p["C"])
            a = (T_["x"], T_["fc_w"], T_["fc_b"])
            for n in self.defect_names():
                out[n] = dict(out={"channels_256_lost": lambda: bg64(*a, keep=ch < 256), "waves_1_3_lost": lambda: bg64(*a, keep=ch % 256 < 64),
                                   "mean_npix_1": lambda: bg64(*a, div=p["npix"] - 1), "f32_sums": lambda: bg64(*a, f32_sums=True)}[n]())
        elif k == "mi":
            for n in self.defect_names():
                out[n] = split_mi(mi64(T_["drv"], T_["src"], T_["bg"], T_["src_down"], defect=n))
        elif k == "fc":
            for n in self.defect_names():
                flow, occ = fc64(T_["x"], T_["drv"], T_["src"], T_["bg"], defect=n)
                out[n] = dict(flow=flow, occ=occ, occ_x0=2 * occ - 1)
        assert tuple(out) == self.defect_names(), (self.name, tuple(out))
        return out


AA_SHAPES = ((4, 37, 50), (4, 70, 132), (8, 136, 72), (2, 33, 35), (3, 50, 49), (1, 7, 5))          # s, H, W
RM_SHAPES = ((9, 17, 1), (17, 9, 15), (24, 40, 10), (13, 20, 10))                                  # h, w, R
BG_SHAPES = ((32, 144, 32), (300, 9, 304), (1024, 4, 1024), (1024, 1, 1040))                       # C, npix, ld
MOTION_SETS = [(fam, h, w, R) for fam, sizes in (("exact", ((9, 17), (17, 33))), ("random", ((9, 17), (17, 33), (24, 40))))
               for h, w in sizes for R in (1, 10, 15)]

CASES = [
    *[Case(f"aa/s{s}_{H}x{W}", "aa", s=s, H=H, W=W, clip=(s, H) == (4, 70)) for s, H, W in AA_SHAPES],
    *[Case(f"rm/{h}x{w}_R{R}", "rm", h=h, w=w, R=R) for h, w, R in RM_SHAPES],
    *[Case(f"bg/C{C}_npix{n}_ld{ld}", "bg", C=C, npix=n, ld=ld) for C, n, ld in BG_SHAPES],
    # c_pad alternates between 4 (R + 1) and 64 so that every R, every size and both families meet both
    *[Case(f"mi/{fam}_{h}x{w}_R{R}_cpad{cp}", "mi", family=fam, h=h, w=w, R=R, c_pad=cp)
      for i, (fam, h, w, R) in enumerate(MOTION_SETS) for cp in ((4 * (R + 1), 64)[(i // 3 + i % 3) % 2],)],
    *[Case(f"fc/{fam}_{h}x{w}_R{R}", "fc", family=fam, h=h, w=w, R=R) for fam, h, w, R in MOTION_SETS],
]


def rm_isotropic():
    """A deliberately isotropic region on a symmetric 9 x 9 grid (covar = a I up to rounding): the eigenvectors are arbitrary there, so
    only A A^T = covar, finiteness and det(affine) < 0 are asked.  -> (rows (h*w, 16), h, w, R, covar64 (1,R,2,2))."""
    h = w = 9
    x = rm_inputs(1, h, w, 2, isotropic=True)
    return wide_rows(x.reshape(-1, 2), LD_ROWS), h, w, 2, mc.region_moments(x, h, w, TEMPERATURE)[1]
