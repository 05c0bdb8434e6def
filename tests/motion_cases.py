"""The LFG motion encode (csrc/motion_encode.hip, dawn_pytorch_amd/motion_encoder.py): its test inputs, a restatement in torch fp64 of the
five definitions of include/dawn_hip.h, and a CPU op set for the orchestration.

Inputs.  `frames_u8(case)` makes the source image and the driving frames of a golden case by an integer formula (bytes, so nothing about
them depends on a platform's floating point): tools/gen_goldens_motion.py feeds exactly these to the reference's modules, and the goldens
hold outputs only.  The tiny models' weights are tests/golden/motion_tiny_sd.npz (fp16 values: exact in fp32).

The restatement follows the reference's formulas (RP = LFG/modules/region_predictor.py, BG = bg_motion_predictor.py, PF =
pixelwise_flow_predictor.py, UTIL = util.py) on float64 tensors; tests/test_motion_cpu.py pins every function here to the reference's own
stage outputs.  The coordinate grid is the reference's fp32 grid, widened: it is an input of the sums, not a result.

Case A is 96 x 96 (h = 24), not the 40 x 40 (h = 10) first asked for: with num_blocks 3 an Hourglass needs h % 8 == 0 -- at h = 10 the
reference's own Decoder fails in torch.cat (10 -> 5 -> 2 -> 1 down, 1 -> 2 -> 4 up against the 5-pixel skip).  24 is the smallest h
that is no power of two and runs: 576 pixels = 2.25 reduction strides of 256, 1.5 x 1.5 antialias tiles, 9 motion-input workgroups."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.ops_ref import RefOps

R = 10
TEMPERATURE = 0.1
S = 4                                        # 1 / scale_factor of both predictors
TINY = dict(block_expansion=8, max_features=32, num_blocks=3)
GEN_TINY = dict(block_expansion=16, max_features=32, num_down_blocks=2, num_bottleneck_blocks=1)      # the generator's own trunk (decode half)
CASES = {"A": dict(H=96, W=96, T=5), "B": dict(H=256, W=256, T=2)}
# End-to-end only (optical_flow and occlusion_map, no stage values): kept apart from CASES, whose tests expect the full stage set.
# N is not square (h = 24, w = 32): a swap of the two sides anywhere between the frames and the latent shows here, and on no square case.
E2E_CASES = {"N": dict(H=96, W=128, T=2)}
GAP_MIN = 1e-3                               # relative eigen-gap below which a region's eigenvectors are not compared
SKIP_CAP = 0.10                              # ... for at most this share of a golden's regions


def frames_u8(case):
    """-> (source (H,W,3) uint8, driving (T,H,W,3) uint8): triangle waves of quadratic forms that drift with the frame index."""
    c = CASES[case] if case in CASES else E2E_CASES[case]
    H, W, T = c["H"], c["W"], c["T"]
    y = np.arange(H, dtype=np.int64).reshape(1, H, 1, 1)
    x = np.arange(W, dtype=np.int64).reshape(1, 1, W, 1)
    ch = np.arange(3, dtype=np.int64).reshape(1, 1, 1, 3)
    t = np.arange(-1, T, dtype=np.int64).reshape(T + 1, 1, 1, 1)         # -1: the source
    cy, cx = H // 2 + 3 * t, W // 3 + 5 * t
    q = ((y - cy) ** 2 * (ch + 2) + (x - cx) ** 2 * (4 - ch) + (x * y * (t + 2)) // 3) * 2040 // (H * W) + 61 * ch + 17 * t
    v = np.abs(q % 510 - 255).astype(np.uint8)
    return v[0], v[1:]


def to_float(u8):
    """uint8 (..., H, W, 3) -> fp32 (..., 3, H, W) in [0, 1]: byte / 255, one correctly rounded division (ToTensor)."""
    t = torch.from_numpy(np.ascontiguousarray(u8)).float() / 255
    return t.movedim(-1, -3).contiguous()


def coordinate_grid(h, w, dtype=torch.float64):
    """UTIL:51-67 in fp32, as float64 (or `dtype`: the fp32 grid is an input in either): (h, w, 2) = (x, y)."""
    x = 2 * (torch.arange(w).float() / (w - 1)) - 1
    y = 2 * (torch.arange(h).float() / (h - 1)) - 1
    return torch.stack((x.view(1, w).expand(h, w), y.view(h, 1).expand(h, w)), 2).to(dtype)


# ---------------------------------------------------------------------------------------------- the five definitions, float64
# (`dtype`: the same restatement in another float type -- float32 is the CPU fp32 baseline of tests/motion_gate.py)
def aa_kernel(s):
    """UTIL:222-247: the fp32 product kernel divided by its fp32 sum, (K, K)."""
    sigma = (s - 1) / 2
    K = 2 * round(sigma * 4) + 1
    if s == 1:
        return torch.ones(1, 1)
    g = torch.exp(-(torch.arange(K, dtype=torch.float32) - (K - 1) / 2) ** 2 / (2 * sigma ** 2))
    k2 = g.view(K, 1) * g.view(1, K)
    return k2 / torch.sum(k2)


def antialias_down(x, s, dtype=torch.float64):
    """UTIL:256-264: x (T,3,H,W) -> (T,3,ceil(H/s),ceil(W/s)) float64."""
    k2 = aa_kernel(s).to(dtype)
    ka = k2.shape[0] // 2
    out = F.conv2d(F.pad(x.to(dtype), (ka, ka, ka, ka)), k2.view(1, 1, *k2.shape).repeat(3, 1, 1, 1), groups=3)
    return out[:, :, ::s, ::s]


def sqrt_factor(covar):
    """U diag(sqrt(s)) of symmetric 2x2 matrices (..., 2, 2) in closed form, include/dawn_hip.h's convention (det U = -1)."""
    a, b, c = covar[..., 0, 0], covar[..., 0, 1], covar[..., 1, 1]
    hd = 0.5 * (a - c)
    rad = torch.sqrt(hd * hd + b * b)
    s1 = 0.5 * (a + c) + rad
    s2 = torch.where(s1 > 0, (a * c - b * b) / s1, torch.zeros_like(s1)).clamp(min=0)
    ux = torch.where(hd >= 0, hd + rad, b)
    uy = torch.where(hd >= 0, b, rad - hd)
    n = torch.sqrt(ux * ux + uy * uy)
    ux, uy = torch.where(n > 0, ux / n, torch.ones_like(n)), torch.where(n > 0, uy / n, torch.zeros_like(n))
    flip = (ux < 0) | ((ux == 0) & (uy < 0))
    ux, uy = torch.where(flip, -ux, ux), torch.where(flip, -uy, uy)
    q1, q2 = torch.sqrt(s1.clamp(min=0)), torch.sqrt(s2)
    return torch.stack((torch.stack((ux * q1, uy * q2), -1), torch.stack((uy * q1, -ux * q2), -1)), -2)


def eigen_gap(covar):
    """(s1 - s2) / s1 of symmetric 2x2 matrices."""
    a, b, c = covar[..., 0, 0].double(), covar[..., 0, 1].double(), covar[..., 1, 1].double()
    rad = torch.sqrt((0.5 * (a - c)) ** 2 + b * b)
    return 2 * rad / (0.5 * (a + c) + rad)


def region_moments(x, h, w, temperature=TEMPERATURE, dtype=torch.float64):
    """RP:84-117 after the `regions` conv: x (T, h*w, R) -> shift (T,R,2), covar (T,R,2,2), affine (T,R,2,2), float64."""
    p = torch.softmax(x.to(dtype) / temperature, dim=1)                              # over the pixels
    g = coordinate_grid(h, w, dtype).reshape(h * w, 2)
    shift = torch.einsum("tpr,pc->trc", p, g)
    d = g.view(1, 1, h * w, 2) - shift.unsqueeze(2)                                  # (T,R,hw,2)
    covar = torch.einsum("tpr,trpa,trpb->trab", p, d, d)
    return shift, covar, sqrt_factor(covar)


def bg_params(last, fc_w, fc_b, dtype=torch.float64):
    """BG:46-52: last (T, npix, C) -> (T,3,3) float64."""
    v = last.to(dtype).mean(dim=1) @ fc_w.to(dtype).t() + fc_b.to(dtype)
    out = torch.eye(3, dtype=dtype).repeat(last.shape[0], 1, 1)
    out[:, :2, :] = v.view(-1, 2, 3)
    return out


def motion_matrix(src_affine, drv_affine, dtype=torch.float64):
    """PF:72-74: A_s . inverse(A_d) times the sign of its [0][0]."""
    M = src_affine.to(dtype) @ torch.inverse(drv_affine.to(dtype))
    return M * torch.sign(M[..., 0:1, 0:1])


def sparse_motions(drv, src, bg, h, w, dtype=torch.float64):
    """PF:66-93: -> (T, R+1, h, w, 2) float64; drv = (shift (T,R,2), covar, affine (T,R,2,2)), src the same without T, bg (T,3,3)."""
    g = coordinate_grid(h, w, dtype)
    T = drv[0].shape[0]
    M = motion_matrix(src[2].unsqueeze(0), drv[2], dtype)                            # (T,R,2,2)
    d = g.view(1, 1, h, w, 2) - drv[0].to(dtype).view(T, -1, 1, 1, 2)
    k = torch.einsum("trab,trhwb->trhwa", M, d) + src[0].to(dtype).view(1, -1, 1, 1, 2)
    gh = torch.cat((g, torch.ones(h, w, 1, dtype=dtype)), 2)
    b = torch.einsum("tab,hwb->thwa", bg.to(dtype), gh)
    return torch.cat(((b[..., :2] / b[..., 2:3]).unsqueeze(1), k), 1)


def gaussian(shift, covar, h, w, dtype=torch.float64):
    """UTIL:22-48 with a covariance: (..., R, 2), (..., R, 2, 2) -> (..., R, h, w)."""
    d = coordinate_grid(h, w, dtype) - shift.to(dtype).unsqueeze(-2).unsqueeze(-2)
    ci = torch.inverse(covar.to(dtype))
    return torch.exp(-0.5 * torch.einsum("...hwa,...ab,...hwb->...hw", d, ci, d))


def motion_inputs(drv, src, bg, src_down, dtype=torch.float64):
    """PF:104-120: src_down (3,h,w) -> the hourglass input (T, (R+1)*4, h, w) float64."""
    _, h, w = src_down.shape
    T = drv[0].shape[0]
    heat = gaussian(drv[0], drv[1], h, w, dtype) - gaussian(src[0], src[1], h, w, dtype).unsqueeze(0)
    heat = torch.cat((torch.zeros(T, 1, h, w, dtype=dtype), heat), 1)                 # (T,R+1,h,w)
    m = sparse_motions(drv, src, bg, h, w, dtype)
    K = m.shape[1]
    warped = F.grid_sample(src_down.to(dtype).view(1, 3, h, w).expand(T * K, 3, h, w), m.reshape(T * K, h, w, 2), mode="bilinear",
                           padding_mode="zeros", align_corners=False).view(T, K, 3, h, w)
    return torch.cat((heat.unsqueeze(2), warped), 2).reshape(T, K * 4, h, w)


def flow_combine(x, drv, src, bg, dtype=torch.float64):
    """PF:124-135: x (T, R+2, h, w) = mask | occlusion conv outputs -> optical_flow (T,h,w,2), occlusion_map (T,1,h,w), float64."""
    T, _, h, w = x.shape
    mask = torch.softmax(x[:, :-1].to(dtype), dim=1)
    m = sparse_motions(drv, src, bg, h, w, dtype)
    return (m * mask.unsqueeze(-1)).sum(dim=1), torch.sigmoid(x[:, -1:].to(dtype))


# ---------------------------------------------------------------------------------------------- layouts
def rows_of(x):
    """(T, C, h, w) -> channels-last rows (T*h*w, C)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def maps_of(rows, T, h, w):
    """rows (T*h*w, C) -> (T, C, h, w)."""
    return rows.reshape(T, h, w, -1).permute(0, 3, 1, 2)


class MotionRefOps(RefOps):
    """RefOps plus the five motion-encode ops (the restatement above, results in the inputs' float type): the CPU op set under which
    MotionEncoder's packing and orchestration are checked against the reference."""

    def antialias_down(self, frames, s, c_pad=16, out=None):
        x = frames.permute(0, 3, 1, 2).double() / 255 if frames.dtype == torch.uint8 else frames
        y = rows_of(antialias_down(x, s))
        res = torch.zeros(y.shape[0], c_pad, dtype=torch.float32 if frames.dtype == torch.uint8 else frames.dtype)
        res[:, :3] = y
        if out is not None:
            out.copy_(res)
            return out
        return res

    def region_moments(self, x, T, h, w, R, temperature):
        return tuple(v.to(x.dtype).contiguous() for v in region_moments(x[:, :R].reshape(T, h * w, R), h, w, temperature))

    def bg_params(self, x, T, fc_w, fc_b):
        return bg_params(x.reshape(T, -1, x.shape[1]), fc_w, fc_b).to(x.dtype)

    def motion_inputs(self, drv, src, bg, src_rows, T, h, w, c_pad):
        y = rows_of(motion_inputs(drv, src, bg, src_rows[:, :3].t().reshape(3, h, w)))
        res = torch.zeros(T * h * w, c_pad, dtype=bg.dtype)
        res[:, :y.shape[1]] = y
        return res

    def flow_combine(self, x, drv, src, bg, T, h, w, grid, conf, conf_x0=False):
        Rn = src[0].shape[0]
        flow, occ = flow_combine(maps_of(x[:, :Rn + 2], T, h, w), drv, src, bg)
        grid.copy_(flow.permute(3, 0, 1, 2))
        conf.copy_(2 * occ[:, 0] - 1 if conf_x0 else occ[:, 0])


# ---------------------------------------------------------------------------------------------- goldens, tolerances
def state_dicts():
    """-> {generator, region_predictor, bg_predictor: state_dict} of tests/golden/motion_tiny_sd.npz, fp32."""
    from conftest import load_golden
    out = {"generator": {}, "region_predictor": {}, "bg_predictor": {}}
    for k, v in load_golden("motion_tiny_sd.npz").items():
        tag, name = k.split("/", 1)
        out[tag][name] = torch.from_numpy(v).float()
    return out


def golden(case):
    from conftest import load_golden
    return {k: torch.from_numpy(v) for k, v in load_golden(f"motion_{case}.npz").items()}


def region_params(g, who):
    """(shift, covar, affine) of the golden's `src` or `drv` parameters."""
    return g[f"{who}_shift"], g[f"{who}_covar"], g[f"{who}_affine"]


def assert_close(got, want, what, scale=1.0):
    """The project tolerance, per element: |got - want| <= 1e-4 * max(1, |want|) * scale."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    bound = 1e-4 * want.abs().clamp(min=1.0) * scale
    worst = float((err / bound).max())
    print(f"{what}: max |err| {float(err.max()):.3g}, worst err / bound {worst:.3g}")
    assert bool((err <= bound).all()), (what, float(err.max()), worst)


def assert_gate(got, ref32, want64, what, c=5.0):
    """Kernel error against float64 <= c x the error of the reference's own fp32 result against the same float64 (max norm)."""
    e_got = float((got.double().cpu() - want64).abs().max())
    e_ref = float((ref32.double() - want64).abs().max())
    print(f"{what}: kernel vs fp64 {e_got:.3g}, reference fp32 vs fp64 {e_ref:.3g}, ratio {e_got / e_ref if e_ref else float('inf'):.3g}")
    assert e_got <= c * e_ref, (what, e_got, e_ref)


def check_affine(aff, covar, what):
    """A . A^T = covar at the project tolerance."""
    a = aff.double().cpu()
    assert_close(a @ a.transpose(-1, -2), covar, what + ": A A^T = covar")


def check_motion_matrices(aff_s, aff_d, g_s, g_d, what):
    """M = A_s . inverse(A_d) after the sign fix against the golden pair's, at the project tolerance over the smaller relative eigen-gap of
    the two covariances (the condition bound of the eigenvectors); regions below GAP_MIN or with det(u) > 0 in the reference are skipped,
    at most SKIP_CAP of them.  g_s / g_d = (covar, affine, u) of the golden."""
    M = motion_matrix(aff_s.cpu(), aff_d.cpu())
    Mg = motion_matrix(g_s[1], g_d[1])
    gap = torch.minimum(eigen_gap(g_s[0]).expand(Mg.shape[:-2]), eigen_gap(g_d[0]).expand(Mg.shape[:-2]))
    skip = (gap < GAP_MIN) | (torch.det(g_s[2]).expand(gap.shape) > 0) | (torch.det(g_d[2]).expand(gap.shape) > 0)
    assert float(skip.float().mean()) <= SKIP_CAP, (what, int(skip.sum()))
    err = (M - Mg).abs().amax(dim=(-1, -2))
    bound = 1e-4 * Mg.abs().amax(dim=(-1, -2)).clamp(min=1.0) / gap
    print(f"{what}: {int(skip.sum())} of {skip.numel()} regions skipped, max |M - M_ref| {float(err[~skip].max()):.3g}, worst err / bound "
          f"{float((err / bound)[~skip].max()):.3g}, min gap {float(gap.min()):.3g}")
    assert bool((err <= bound)[~skip].all()), what
