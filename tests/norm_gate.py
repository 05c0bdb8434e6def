"""The fp32-accuracy gate of tests/split_gate.py on every launch branch of the streaming kernels between the matrix kernels: GroupNorm
statistics / apply and the per-pixel LayerNorm (csrc/norm.hip) and the boundary kernels init_conv_x* and head_out (csrc/misc.hip).  The
gate, its factor and its floor are split_gate's:

    rel_err(got) <= c * rel_err(base32) + FLOOR,      rel_err(t) = max|t - want64| / max|want64|,      c = C_GATE unless C_WIDE widens it,

want64 = the op in float64 on the CPU; base32 = the same op carried out in float32 on the CPU, so that it has a true fp32 error:
GroupNorm with fp32 sums (RefOps.gn_coeffs sums in float64 and is NOT base32; it is the `reference arithmetic` that
test_norm_gate_cpu holds inside the gate), LayerNorm through torch's fp32 mean / var, init_conv_x through decode_gate's im2col path,
head_out as an fp32 matmul.  A case's result is a dict of named outputs; each output is checked in one of three modes (`Case.mode`):
"gate" (the inequality above), "floor" (rel_err <= FLOOR: the 16 fp64 GroupNorm sums) and "exact" (torch.equal: dawn_gn_reduce on
integer-valued partials, where every summation order gives the same bits).

tests/test_norm_gate_cpu.py shows on the CPU that every case accepts base32 and rejects each defect of `Case.defect_names()` on every
output the defect reaches, emulated in float64 against the same want64 and checked with the case's own c, and that every emulator
without a defect is the plain reference.  tests/test_hip_norm_fp64_gates.py runs the same cases on the GPU kernels.

The data is seeded and NOT i.i.d.: on i.i.d. rows a GroupNorm that loses a block of rows or credits a channel to the wrong group still
finds nearly the right mean and variance.  GroupNorm inputs (`gn_data`) carry an amplitude ramp over the rows and a distinct offset per
channel; LayerNorm rows (`ln_data`) a per-row DC offset of std 3 and a per-row amplitude in [0.25, 2], the regime in which a one-pass
variance fails; init_conv_x and head_out the magnitudes of decode_gate and test_hip_heads_eps.

The thresholds below are the kernels' own (csrc/norm.hip, csrc/misc.hip); the cases sit on both sides of each.

kind "gn_stats"   dawn_gn_partial -> dawn_gn_reduce_finalize, and -> dawn_gn_reduce + dawn_gn_finalize.  `nblk` None: the grid
                  HipOps.gn_coeffs chooses (`gn_nblk`); else dawn_gn_partial is launched with that many blocks, which reaches the flush
                  of the fp32 runs every GN_RUN = 64 rows per thread with kilobytes of data (n = rows per thread).  Defects: the
                  remainder after a thread's last full run of 64 lost (`gn_partial_emul`, the kernel's thread-to-row map; below 64 rows
                  per thread that is every row); the four channels of a quad credited to the first channel's group (C = 8, 16: a quad
                  spans groups); ld taken as C on a column slice; the FiLM shift applied before the scale; the count taken from this
                  call's rows where total_rows differs.
kind "gn_reduce"  gn_reduce_block<NT> on integer-valued float64 partials.  NP = NT / 16 row phases; the 16-way unrolled loop runs for
                  nblk > 15 NP (240 for dawn_gn_reduce_finalize, 960 for dawn_gn_reduce), the scalar tail takes the rest (`in_unrolled`).
                  Defects: the tail dropped; the unrolled rounds dropped.  Each reaches an output only where its kernel has such rows
                  (at nblk = 1024 neither kernel has a tail).
kind "gn_apply"   gn_apply_res: the grid is capped at 8192 blocks of 256; the grid-stride loop's second trip starts at quad 2,097,152.
                  Defect (cases past it): the quads of the second trip left as the input.  The other cases carry none: the CPU test checks
                  that base32 has a real fp32 error on them.
kind "ln"         ln_rowstats / ln_rows: L = min(64, C / 4 rounded down to a power of two, at least 4) lanes per row, R = 4 rows per
                  lane group from 65536 rows.  Defects: the variance in one fp32 pass; the second source's columns read from the first;
                  the padding quads (qd >= C / 4, every width below 16 L) entering the squared deviations as (0 - mean)^2; on R = 4
                  launches row 4 g + r written to row r * ceil(rows / 4) + g (the R = 1 mapping) and the last rows % 4 rows left zero.
kind "first"      init_conv_x: the persistent MFMA kernel (Co = 64, 256 % w == 0, h a multiple of 256 / w; at most FIRST_SLOTS = 768
                  workgroups) and the generic one (grid-stride from 4096 x 256 threads).  Defects: decode_gate's three (weights
                  truncated to 16 mantissa bits, last tap lost, wrapped patch); a workgroup's later tiles computed from its first tile's
                  patch; the plane stride taken as F_sub h w on a frame sub-range.
kind "head"       head_out at Co = 128 and 256 (the `c += 64` loop runs 2 and 4 times), both heads and each alone into a pre-filled
                  buffer.  Defects: the channels from 64 up lost; the absent head's rows written (as bias only)."""
import torch
import torch.nn.functional as F_

from decode_gate import _cpu_fp32, rnd, trunc16
from oracle.ops_ref import RefOps
from split_gate import C_GATE, FLOOR, LOG, coherent, fp32_gate, gate_rejects, rel_err  # noqa: F401 (re-exported)

EPS = 1e-5
GN_RUN = 64                         # gn_partial_kernel: rows per thread between two flushes of the fp32 runs into fp64
GN_APPLY_QUADS = 8192 * 256         # gn_apply_res_kernel: quads of one grid-wide trip
LN_R4_ROWS = 65536                  # ln_launch: R = 4 from this many rows
FIRST_SLOTS = 768                   # init_conv_x_mfma_kernel: workgroups at most
FIRST_GENERIC_THREADS = 4096 * 256  # init_conv_x_kernel: threads of one grid-wide trip

# Gate factors widened past C_GATE: GPU error / CPU fp32 error against float64 measured on an MI355X (max over that kernel's cases), x 1.5,
# rounded up to the next 0.5 (the rule of stage_gate.C_WIDE).  Empty: every kernel of this file holds C_GATE = 2.  Measured maxima
# (profiles/norm_gate_ratios.md names the cases): gn_partial -> gn_reduce_finalize 0.78, -> gn_reduce + gn_finalize 0.78 (the 16 sums
# within 2.4e-8 of float64); gn_reduce_finalize on integer partials 1.29; gn_apply_res 1.01; ln_rowstats R = 1 1.61 (rstd; rows 1.52),
# R = 4 1.17 (rstd; rows 0.84); init_conv_x_mfma 1.32; init_conv_x 1.40; head_out 0.92.  The narrowest gate: the rows of ln/r203_C28 at 0.67
# of their bound.
C_WIDE = {
}


# ---------------------------------------------------------------------------------------------- data
def gn_data(rows, width, seed=1):
    """(rows, width) float32: N(0, 1) x an amplitude ramp 0.5 .. 2 over the rows + a distinct offset per channel."""
    r = torch.arange(rows, dtype=torch.float32)[:, None]
    c = torch.arange(width, dtype=torch.float32)[None]
    off = ((7 * c) % 16 - 7.5) * 0.2 + c / width * 0.5
    return rnd(rows, width, seed=seed) * (0.5 + 1.5 * r / max(rows - 1, 1)) + off


def ln_data(rows, width, seed=1):
    """(rows, width) float32: per row a DC offset of std 3 and an amplitude in [0.25, 2]."""
    g = torch.Generator().manual_seed(seed)
    amp = 0.25 + 1.75 * torch.rand(rows, 1, generator=g)
    return torch.randn(rows, width, generator=g) * amp + torch.randn(rows, 1, generator=g) * 3.0


# ---------------------------------------------------------------------------------------------- GroupNorm references
def gn_nblk(rows, C):
    """The grid of HipOps.gn_coeffs' statistics pass."""
    return max(1, min(1024, (rows * (C // 4) + 255) // 256 // 8))


def group_sums(x, dtype):
    """[sum, sumsq] of the 8 channel groups of x (rows, C), summed in dtype -> (16,) of dtype."""
    rows, C = x.shape
    xg = x.to(dtype).reshape(rows, 8, C // 8)
    return torch.stack((xg.sum(dim=(0, 2)), (xg * xg).sum(dim=(0, 2))), dim=1).reshape(16)


def gn_partial_emul(x, nblk, dtype=torch.float64, lose_remainder=False, quad_first=False):
    """The 16 sums through gn_partial_kernel's thread-to-row map: thread (block, r0, cq) owns channel quad cq of the rows
    block * rpb + r0 + k * nblk * rpb.  dtype float32: the kernel's arithmetic (fp32 runs of GN_RUN rows, flushed into fp64); float64: the
    plain sums in another order.  lose_remainder: the add after the loop is missing (the rows after a thread's last full run);
    quad_first: all four channels of a quad go to the group of its first channel."""
    rows, C = x.shape
    rpb = 256 // (C // 4)
    stride = nblk * rpb
    K = -(-rows // stride)
    xs = torch.zeros(K * stride, C, dtype=dtype)
    xs[:rows] = x.to(dtype)
    xs = xs.view(K, stride, C)
    cnt = torch.full((stride,), K - 1) + (torch.arange(stride) < rows - (K - 1) * stride).long()      # rows each thread slot sees
    ds = torch.zeros(stride, C, dtype=torch.float64)
    dss = torch.zeros(stride, C, dtype=torch.float64)
    s = torch.zeros(stride, C, dtype=dtype)
    ss = torch.zeros(stride, C, dtype=dtype)
    for k in range(K):
        s, ss = s + xs[k], ss + xs[k] * xs[k]
        if (k + 1) % GN_RUN == 0:
            full = (cnt > k)[:, None]                    # (a slot whose rows ended before k never counted up to 64 here)
            ds, dss = ds + torch.where(full, s.double(), 0.0), dss + torch.where(full, ss.double(), 0.0)
            s, ss = torch.where(full, 0.0, s), torch.where(full, 0.0, ss)
    if not lose_remainder:
        ds, dss = ds + s.double(), dss + ss.double()
    ch = torch.arange(C)
    g = ((ch // 4 * 4) if quad_first else ch) // (C // 8)
    out = torch.zeros(8, 2, dtype=torch.float64)
    out[:, 0].index_add_(0, g, ds.sum(0))
    out[:, 1].index_add_(0, g, dss.sum(0))
    return out.reshape(16)


def gn_coeff(sums, count, gamma, beta, fs, fsh, fp32_final, shift_first=False):
    """gn_coeff of csrc/norm.hip on 16 sums.  fp32_final: mean, variance in float64, then rstd, mu and everything after them in float32
    (the kernel's arithmetic) -> float32; else everything in float64.  shift_first: the FiLM shift added before the scale."""
    C = gamma.numel()
    sums = sums.double().reshape(8, 2)
    mean = sums[:, 0] / count
    var = (sums[:, 1] / count - mean * mean).clamp(min=0)
    dt = torch.float32 if fp32_final else torch.float64
    rstd = (1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))).to(dt).repeat_interleave(C // 8)
    mu = mean.to(dt).repeat_interleave(C // 8)
    a = rstd * gamma.to(dt)
    b = beta.to(dt) - mu * a
    if fs is not None:
        sc = fs.to(dt) + 1.0
        a = a * sc
        b = (b + fsh.to(dt)) * sc if shift_first else b * sc + fsh.to(dt)
    return a, b


def in_unrolled(nblk, NT):
    """gn_reduce_block<NT>: (nblk,) bool, True for the partial rows its 16-way unrolled loop adds (thread phase r = row % NP runs a round
    while r + 16 NP k + 15 NP < nblk), False for those of the scalar tail."""
    NP = NT // 16
    b = torch.arange(nblk)
    rounds = ((nblk - 1 - 15 * NP - b % NP) // (16 * NP) + 1).clamp(min=0)
    return b // NP < 16 * rounds


# ---------------------------------------------------------------------------------------------- LayerNorm reference
def ln_lanes(C):
    nq = C // 4
    return 64 if nq >= 64 else 32 if nq >= 32 else 16 if nq >= 16 else 8 if nq >= 8 else 4


def _flat_rows(wide, start, ld, rows, n):
    """rows x n values read from wide's memory at start + r * ld + j (zero behind the buffer)."""
    flat = torch.cat((wide.reshape(-1), torch.zeros(ld + n, dtype=wide.dtype)))
    idx = start + torch.arange(rows)[:, None] * ld + torch.arange(n)[None]
    return flat[idx.clamp_max(flat.numel() - 1)]


def ln64(T_, p, defect=None):
    """ln_rowstats / ln_rows in float64 -> {mean, rstd, xn}; defect: None, "onepass32", "second_from_first" or "pad_quads"."""
    x0 = T_["w0"][:, p["o0"]:p["o0"] + p["C0"]].double()
    C1 = p.get("C1", 0)
    if C1 and defect == "second_from_first":
        x1 = _flat_rows(T_["w0"], p["o0"], T_["w0"].shape[1], x0.shape[0], C1).double()
    elif C1:
        x1 = T_["w1"][:, p["o1"]:p["o1"] + C1].double()
    x = torch.cat((x0, x1), dim=1) if C1 else x0
    C = x.shape[1]
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    if defect == "pad_quads":
        var = var + (4 * ln_lanes(C) - C // 4) * 4 * mean * mean / C
    if defect == "onepass32":
        x32 = x.float()
        m32 = x32.sum(dim=1) / C
        var = ((x32 * x32).sum(dim=1) / C - m32 * m32).double().clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return dict(mean=mean, rstd=rstd, xn=(x - mean[:, None]) * rstd[:, None])


# ---------------------------------------------------------------------------------------------- cases
class Case:
    """name, kind, parameters.  make() -> the seeded float32 inputs; want64 / base32 -> {output: tensor}; defects() -> {name: {output the
    defect reaches: result of the defective op in float64}}."""

    def __init__(self, name, kind, **p):
        self.name, self.kind, self.p = f"{kind}/{name}", kind, p
        self.c = C_WIDE.get(self.kernel(), C_GATE)

    def __repr__(self):
        return self.name

    def kernel(self):
        """The kernel whose measured ratio (C_WIDE, profiles/norm_gate_ratios.md) this case counts towards."""
        if self.kind == "first":
            return "init_conv_x_mfma" if self.mfma() else "init_conv_x"
        return {"gn_stats": "gn_partial", "gn_reduce": "gn_reduce_finalize", "gn_apply": "gn_apply_res", "ln": "ln_rowstats",
                "head": "head_out"}[self.kind]

    @staticmethod
    def mode(key):
        return {"sums": "floor", "sums_exact": "exact"}.get(key, "gate")

    def rejects(self, key, t, want64, base32):
        """Does the check of output `key` reject t?"""
        m = self.mode(key)
        if m == "exact":
            return not torch.equal(t.double().cpu(), want64[key])
        if m == "floor":
            return rel_err(t, want64[key]) > FLOOR
        return gate_rejects(t, want64[key], base32[key], c=self.c)

    def check(self, key, got, want64, base32, tag=""):
        """Assert the check of output `key` on a GPU result (gated outputs append their record to the op-error log); tag: the launch path,
        where a case runs more than one."""
        m, name = self.mode(key), f"{self.name}/{tag}{key}"
        if m == "exact":
            assert torch.equal(got.cpu().double(), want64[key]), f"{name}: not bit-identical to the exact sums"
        elif m == "floor":
            e = rel_err(got, want64[key])
            print(f"{name}: rel err {e:.3e}")
            assert e <= FLOOR, f"{name}: rel err {e:.3e} > {FLOOR:.0e}"
        else:
            return fp32_gate(name, got, want64[key], base32[key], c=self.c)

    # ------------------------------------------------------------------ geometry
    def nblk(self):
        p = self.p
        return p["nblk"] if p.get("nblk") else gn_nblk(p["rows"], p["C"])

    def thread_rows(self):
        """gn_stats: the row counts the threads of gn_partial_kernel see (one or two distinct values; 0 for blocks without rows)."""
        stride = self.nblk() * (256 // (self.p["C"] // 4))
        K, left = divmod(self.p["rows"], stride)
        return {K + 1, K} if left else {K}

    def lanes(self):
        return ln_lanes(self.p["C0"] + self.p.get("C1", 0))

    def r4(self):
        return self.p["rows"] >= LN_R4_ROWS

    def mfma(self):
        p = self.p
        h, w = p["h"], p["w"]
        return p.get("Co", 64) == 64 and w <= 256 and 256 % w == 0 and h % (256 // w) == 0

    def fsub(self):
        fa, fb = self.p.get("frames") or (0, self.p["F"])
        return fa, fb

    def tiles(self):
        """first: (tiles, tiles per frame) of the MFMA launch."""
        p = self.p
        tpf = p["h"] // (256 // p["w"])
        fa, fb = self.fsub()
        return (fb - fa) * tpf, tpf

    def threads(self):
        """first: the generic kernel's threads (pixels x Co / 4)."""
        p = self.p
        fa, fb = self.fsub()
        return (fb - fa) * p["h"] * p["w"] * (p.get("Co", 64) // 4)

    def x_of(self, T_):
        p = self.p
        return T_["wide"][:, p.get("off", 0):p.get("off", 0) + p["C"]]

    # ------------------------------------------------------------------ inputs
    def make(self):
        p, k = self.p, self.kind
        if k == "gn_stats":
            C = p["C"]
            film = p.get("film")
            return dict(wide=gn_data(p["rows"], p.get("ld", C)), gamma=rnd(C, seed=2) * 0.2 + 1, beta=rnd(C, seed=3) * 0.2,
                        fs=rnd(C, seed=4) * 0.3 if film else None, fsh=rnd(C, seed=5) * 0.3 if film else None)
        if k == "gn_reduce":
            n, C = p["nblk"], 64
            g = torch.Generator().manual_seed(n)
            part = torch.stack((torch.randint(-500, 1501, (n, 8), generator=g), torch.randint(1000000, 2000001, (n, 8), generator=g)),
                               dim=2).reshape(n, 16).double()
            return dict(part=part, gamma=rnd(C, seed=2) * 0.2 + 1, beta=rnd(C, seed=3) * 0.2, fs=rnd(C, seed=4) * 0.3, fsh=rnd(C, seed=5) * 0.3)
        if k == "gn_apply":
            rows, C = p["rows"], p["C"]
            return dict(x=gn_data(rows, C), a=rnd(C, seed=2) * 0.2 + 0.8, b=rnd(C, seed=3) * 0.3, res=rnd(rows, C, seed=6) if p.get("res") else None)
        if k == "ln":
            rows, C1 = p["rows"], p.get("C1", 0)
            ld0, ld1 = p.get("ld0", p["C0"]), p.get("ld1", C1)
            both = ln_data(rows, ld0 + ld1)                # one DC offset and one amplitude per row, over both sources
            return dict(w0=both[:, :ld0].contiguous(), w1=both[:, ld0:].contiguous() if C1 else None)
        if k == "first":
            F, h, w, Co = p["F"], p["h"], p["w"], p.get("Co", 64)
            return dict(x=torch.rand(3, F, h, w, generator=torch.Generator().manual_seed(1)),
                        w3=coherent(rnd(147, Co, seed=2, scale=147 ** -0.5)), fea_pre=rnd(h * w, Co, seed=3, scale=0.1))
        if k == "head":
            rows, Co, which = p["rows"], p["Co"], p["which"]
            return dict(hg=rnd(rows, Co, seed=1) * 1.7 + 0.3 if which != "o" else None, ho=rnd(rows, Co, seed=2) * 0.8 - 0.2 if which != "g" else None,
                        wg=rnd(2, Co, seed=3, scale=Co ** -0.5), bg=rnd(2, seed=4, scale=0.1), wo=rnd(1, Co, seed=5, scale=Co ** -0.5),
                        bo=rnd(1, seed=6, scale=0.1), prefill=None if which == "both" else rnd(3, rows, seed=7))
        raise ValueError(k)

    def ln_sources(self, T_):
        """(in0, in1) as the kernel takes them: the buffers, or column slices of wider ones."""
        p = self.p
        in0 = T_["w0"][:, p.get("o0", 0):p.get("o0", 0) + p["C0"]]
        return in0, (T_["w1"][:, p.get("o1", 0):p.get("o1", 0) + p["C1"]] if p.get("C1") else None)

    # ------------------------------------------------------------------ the references
    def count(self):
        p = self.p
        if self.kind == "gn_reduce":
            return float(p["nblk"]) * 64 * 8
        return float(p.get("total_rows", p["rows"])) * (p["C"] // 8)

    def _ln_p(self):
        p = self.p
        return dict(C0=p["C0"], C1=p.get("C1", 0), o0=p.get("o0", 0), o1=p.get("o1", 0))

    def want64(self, T_):
        k, p = self.kind, self.p
        if k == "gn_stats":
            sums = group_sums(self.x_of(T_), torch.float64)
            a, b = gn_coeff(sums, self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=False)
            return dict(a=a, b=b, sums=sums)
        if k == "gn_reduce":
            sums = T_["part"].sum(dim=0)
            a, b = gn_coeff(sums, self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=False)
            return dict(a=a, b=b, sums_exact=sums)
        if k == "gn_apply":
            y = F_.silu(T_["x"].double() * T_["a"].double() + T_["b"].double())
            return dict(y=y if T_["res"] is None else y + T_["res"].double())
        if k == "ln":
            return ln64(T_, self._ln_p())
        if k == "first":
            return dict(out=RefOps().init_conv_x(T_["x"].double(), T_["w3"].double(), T_["fea_pre"].double(), p["F"], p["h"], p["w"],
                                                 p.get("Co", 64), frames=p.get("frames")))
        if k == "head":
            return dict(eps=self._head(T_, torch.float64))
        raise ValueError(k)

    def base32(self, T_):
        k, p = self.kind, self.p
        if k == "gn_stats":
            a, b = gn_coeff(group_sums(self.x_of(T_), torch.float32), self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=True)
            return dict(a=a, b=b)
        if k == "gn_reduce":
            a, b = gn_coeff(T_["part"].float().sum(dim=0), self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=True)
            return dict(a=a, b=b)
        if k == "gn_apply":
            y = F_.silu(T_["x"] * T_["a"] + T_["b"])
            return dict(y=y if T_["res"] is None else y + T_["res"])
        if k == "ln":
            in0, in1 = self.ln_sources(T_)
            mean, rstd = RefOps().ln_rowstats(in0, in1, EPS)
            return dict(mean=mean, rstd=rstd, xn=RefOps().ln_rows(in0, in1, EPS))
        if k == "first":
            return dict(out=_cpu_fp32(lambda: RefOps().init_conv_x(T_["x"], T_["w3"], T_["fea_pre"], p["F"], p["h"], p["w"], p.get("Co", 64),
                                                                   frames=p.get("frames"))))
        if k == "head":
            return dict(eps=self._head(T_, torch.float32))
        raise ValueError(k)

    def reference_arithmetic(self, T_):
        """gn_stats: float64 sums, then the fp32 finalisation of gn_coeff -- what a faultless kernel computes."""
        a, b = gn_coeff(group_sums(self.x_of(T_), torch.float64), self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=True)
        return dict(a=a, b=b)

    def _head(self, T_, dtype, hi_lost=False, absent_written=False):
        t = {n: (None if v is None else v.to(dtype)) for n, v in T_.items()}
        rows = self.p["rows"]
        if hi_lost:
            t = {n: (v if v is None or n not in ("wg", "wo") else torch.cat((v[:, :64], torch.zeros_like(v[:, 64:])), dim=1)) for n, v in t.items()}
        out = t["prefill"].clone() if t["prefill"] is not None else torch.empty(3, rows, dtype=dtype)
        if t["hg"] is not None:
            out[:2] = (t["hg"] @ t["wg"].t() + t["bg"]).t()
        elif absent_written:
            out[:2] = t["bg"][:, None].expand(2, rows)
        if t["ho"] is not None:
            out[2:] = (t["ho"] @ t["wo"].t() + t["bo"]).t()
        elif absent_written:
            out[2:] = t["bo"][:, None].expand(1, rows)
        return out

    # ------------------------------------------------------------------ the defects (see the module docstring)
    def defect_names(self):
        k, p = self.kind, self.p
        if k == "gn_stats":
            return ((("remainder_lost",) if any(n % GN_RUN for n in self.thread_rows()) else ())
                    + (("quad_to_first_group",) if p["C"] < 32 else ()) + (("ld_as_C",) if p.get("ld", p["C"]) > p["C"] else ())
                    + (("film_shift_first",) if p.get("film") else ()) + (("count_from_rows",) if p.get("total_rows", p["rows"]) != p["rows"] else ()))
        if k == "gn_reduce":
            n = p["nblk"]
            tail = not bool(in_unrolled(n, 256).all()) or not bool(in_unrolled(n, 1024).all())
            return (("tail_dropped",) if tail else ()) + (("unrolled_dropped",) if bool(in_unrolled(n, 256).any()) else ())
        if k == "gn_apply":
            return ("second_trip_lost",) if p["rows"] * (p["C"] // 4) > GN_APPLY_QUADS else ()
        if k == "ln":
            C = p["C0"] + p.get("C1", 0)
            return (("onepass32",) + (("second_from_first",) if p.get("C1") else ()) + (("pad_quads",) if C // 4 < 4 * ln_lanes(C) else ())
                    + (("r4_rows_as_r1",) if self.r4() else ()) + (("r4_tail_zero",) if self.r4() and p["rows"] % 4 else ()))
        if k == "first":
            return (("trunc16", "last_tap_lost", "wrapped_patch") + (("stale_patch",) if self.mfma() and self.tiles()[0] > FIRST_SLOTS else ())
                    + (("plane_stride",) if p.get("frames") else ()))
        if k == "head":
            return ("channels_from_64_lost",) + (("absent_head_written",) if p["which"] != "both" else ())
        raise ValueError(k)

    def defects(self, T_, want64):
        k, p = self.kind, self.p
        names, out = self.defect_names(), {}
        if k == "gn_stats":
            x, cnt = self.x_of(T_), self.count()
            co = lambda sums, **kw: gn_coeff(sums, kw.pop("count", cnt), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"], fp32_final=False, **kw)  # noqa: E731

            def stats(sums):
                a, b = co(sums)
                return dict(a=a, b=b, sums=sums)
            if "remainder_lost" in names:
                out["remainder_lost"] = stats(gn_partial_emul(x, self.nblk(), lose_remainder=True))
            if "quad_to_first_group" in names:
                out["quad_to_first_group"] = stats(gn_partial_emul(x, self.nblk(), quad_first=True))
            if "ld_as_C" in names:
                C = p["C"]
                out["ld_as_C"] = stats(group_sums(_flat_rows(T_["wide"], p["off"], C, p["rows"], C), torch.float64))
            if "film_shift_first" in names:
                out["film_shift_first"] = dict(b=co(want64["sums"], shift_first=True)[1])
            if "count_from_rows" in names:
                a, b = co(want64["sums"], count=float(p["rows"]) * (p["C"] // 8))
                out["count_from_rows"] = dict(a=a, b=b)
        elif k == "gn_reduce":
            part, n = T_["part"], p["nblk"]
            for name, keep_unrolled in (("tail_dropped", True), ("unrolled_dropped", False)):
                if name not in names:
                    continue
                o = {}
                m1024, m256 = in_unrolled(n, 1024), in_unrolled(n, 256)
                if not bool((m1024 == keep_unrolled).all()):                  # dawn_gn_reduce (NT = 1024) has rows of the dropped kind
                    o["sums_exact"] = part[m1024 == keep_unrolled].sum(dim=0)
                if not bool((m256 == keep_unrolled).all()):                   # dawn_gn_reduce_finalize (NT = 256)
                    o["a"], o["b"] = gn_coeff(part[m256 == keep_unrolled].sum(dim=0), self.count(), T_["gamma"], T_["beta"], T_["fs"], T_["fsh"],
                                              fp32_final=False)
                out[name] = o
        elif k == "gn_apply":
            if names:
                y = want64["y"].clone()
                y.view(-1)[GN_APPLY_QUADS * 4:] = T_["x"].double().view(-1)[GN_APPLY_QUADS * 4:]
                out["second_trip_lost"] = dict(y=y)
        elif k == "ln":
            lp, rows = self._ln_p(), p["rows"]
            d = ln64(T_, lp, "onepass32")
            out["onepass32"] = dict(rstd=d["rstd"], xn=d["xn"])
            if "second_from_first" in names:
                out["second_from_first"] = ln64(T_, lp, "second_from_first")
            if "pad_quads" in names:
                d = ln64(T_, lp, "pad_quads")
                out["pad_quads"] = dict(rstd=d["rstd"], xn=d["xn"])
            if "r4_rows_as_r1" in names:
                ng = -(-rows // 4)
                src = torch.arange(rows)
                dst = (src % 4) * ng + src // 4
                ok = dst < rows
                o = {}
                for key, t in want64.items():
                    o[key] = torch.zeros_like(t)
                    o[key][dst[ok]] = t[src[ok]]
                out["r4_rows_as_r1"] = o
            if "r4_tail_zero" in names:
                o = {key: t.clone() for key, t in want64.items()}
                for t in o.values():
                    t[rows - rows % 4:] = 0
                out["r4_tail_zero"] = o
        elif k == "first":
            F, h, w, Co = p["F"], p["h"], p["w"], p.get("Co", 64)
            fa, fb = self.fsub()
            x, w3, fp = T_["x"].double(), T_["w3"].double(), T_["fea_pre"].double()
            ref = lambda **o: RefOps().init_conv_x(o.get("x", x), o.get("w3", w3), fp, o.get("F", F), h, w, Co, frames=o.get("frames", p.get("frames")))  # noqa: E731
            out["trunc16"] = dict(out=ref(w3=trunc16(T_["w3"])))
            lost = w3.clone()
            lost[-3:] = 0                                               # tap (6, 6), three channels
            out["last_tap_lost"] = dict(out=ref(w3=lost))
            img = x[:, fa:fb]                                           # (3, Fs, h, w)
            pad = F_.pad(img, (3, 3, 3, 3))
            pad[:, :, 3:3 + h - 1, w + 3:] = img[:, :, 1:, :3]          # right padding of row y = the first pixels of row y + 1
            y = F_.conv2d(pad.permute(1, 0, 2, 3), w3.reshape(7, 7, 3, Co).permute(3, 2, 0, 1)).permute(0, 2, 3, 1)
            out["wrapped_patch"] = dict(out=(y.reshape(fb - fa, h * w, Co) + fp[None]).reshape(-1, Co))
            if "stale_patch" in names:
                # tile t >= FIRST_SLOTS convolves the patch of tile t - FIRST_SLOTS (the first of its workgroup), adds its own fea_pre rows and
                # writes its own rows: (want - fea_pre) moved by FIRST_SLOTS tiles
                ntiles, tpf = self.tiles()
                assert tpf == 1                                         # (a tile further down the frame would also differ in its padding)
                conv = (want64["out"].view(fb - fa, h * w, Co) - fp[None]).reshape(ntiles, 256, Co).clone()
                conv[FIRST_SLOTS:] = conv[:ntiles - FIRST_SLOTS].clone()
                out["stale_patch"] = dict(out=(conv.view(fb - fa, h * w, Co) + fp[None]).reshape(-1, Co))
            if "plane_stride" in names:
                Fs = fb - fa
                flat = torch.cat((x.reshape(-1)[fa * h * w:], torch.zeros(3 * Fs * h * w, dtype=x.dtype)))
                xs = torch.stack([flat[c * Fs * h * w:(c + 1) * Fs * h * w] for c in range(3)]).view(3, Fs, h, w)
                out["plane_stride"] = dict(out=ref(x=xs, F=Fs, frames=None))
        elif k == "head":
            out["channels_from_64_lost"] = dict(eps=self._head(T_, torch.float64, hi_lost=True))
            if "absent_head_written" in names:
                out["absent_head_written"] = dict(eps=self._head(T_, torch.float64, absent_written=True))
        assert tuple(out) == names, (self.name, tuple(out))
        return out


def _flush(C, nblk, n):
    """dawn_gn_partial on nblk blocks with exactly n rows per thread."""
    return Case(f"flush_C{C}_nblk{nblk}_n{n}", "gn_stats", C=C, rows=nblk * (256 // (C // 4)) * n, nblk=nblk, n=n, film=n in (64, 65, 128))


REDUCE_NBLK = (1, 15, 16, 17, 240, 241, 256, 257, 511, 960, 961, 1024, 1025, 3200)
R4 = LN_R4_ROWS

CASES = [
    # ---- gn_stats through the grid of HipOps.gn_coeffs: C = 8, 16 a quad spans four / two groups; C = 1024 one row per block iteration
    Case("C16_r4099_film", "gn_stats", C=16, rows=4099, film=True),
    Case("C64_r3000", "gn_stats", C=64, rows=3000),
    Case("C512_r333_film", "gn_stats", C=512, rows=333, film=True),
    Case("C8_r70000", "gn_stats", C=8, rows=70000),
    Case("C1024_r65_film", "gn_stats", C=1024, rows=65, film=True),
    Case("C32_r1001_total1500_film", "gn_stats", C=32, rows=1001, total_rows=1500, film=True),
    Case("C32_r1001_ld48", "gn_stats", C=32, rows=1001, ld=48, off=8),                    # columns 8 .. 40 of a 48-wide buffer
    Case("C16_r200_nblk8", "gn_stats", C=16, rows=200, nblk=8),                           # rpb = 64: block 3 holds 8 rows, blocks 4 .. 7 none
    # ---- the flush of the fp32 runs: 63, 64, 65, 128, 130 rows per thread
    *[_flush(64, 2, n) for n in (63, 64, 65, 128, 130)],
    _flush(1024, 1, 65),
    _flush(8, 1, 130),
    # ---- gn_reduce_block<256> (unrolled from 241) and <1024> (from 961)
    *[Case(f"nblk{n}", "gn_reduce", nblk=n) for n in REDUCE_NBLK],
    # ---- gn_apply_res: one trip (8192 x 256 quads = 32768 rows of 256 channels) and the second one
    Case("C256_r32767_res", "gn_apply", C=256, rows=32767, res=True),
    Case("C256_r32768", "gn_apply", C=256, rows=32768),
    Case("C256_r32769_res", "gn_apply", C=256, rows=32769, res=True),
    Case("C256_r32769_inplace", "gn_apply", C=256, rows=32769, inplace=True),
    Case("C8_r777_res", "gn_apply", C=8, rows=777, res=True),
    Case("C8_r1048579_res_inplace", "gn_apply", C=8, rows=1048579, res=True, inplace=True),
    # ---- LayerNorm: both R forms at C = 16 (the R = 4 tail holds 1 and 3 rows), R = 4 at the other widths
    *[Case(f"r{rows}_C16", "ln", rows=rows, C0=16) for rows in (R4 - 1, R4, R4 + 1, R4 + 3)],
    Case(f"r{R4 + 2}_C96", "ln", rows=R4 + 2, C0=96),                                     # nq = 24 on L = 16
    Case(f"r{R4 + 1}_C48+80", "ln", rows=R4 + 1, C0=48, C1=80),                           # C0 / 4 = 12 on L = 32
    Case(f"r{R4}_C64+64", "ln", rows=R4, C0=64, C1=64),
    Case(f"r{R4 + 3}_C256", "ln", rows=R4 + 3, C0=256),
    # small row counts, no multiple of the rows per block
    Case("r301_C8+8", "ln", rows=301, C0=8, C1=8),
    Case("r203_C24", "ln", rows=203, C0=24),                                              # L = 4: a second quad on lanes 0, 1
    Case("r203_C28", "ln", rows=203, C0=28),
    Case("r203_C40", "ln", rows=203, C0=40),                                              # L = 8, nq = 10
    Case("r131_C1020", "ln", rows=131, C0=1020),
    Case("r131_C512+512", "ln", rows=131, C0=512, C1=512),
    Case("r301_C48+80_ld64+96", "ln", rows=301, C0=48, C1=80, ld0=64, o0=8, ld1=96, o1=4),
    # ---- init_conv_x
    Case("mfma_768x8x32", "first", F=768, h=8, w=32),                                     # one tile for each of the 768 workgroups
    Case("mfma_770x8x32", "first", F=770, h=8, w=32),                                     # 770 tiles on 768 workgroups
    Case("mfma_w8_2x64x8", "first", F=2, h=64, w=8),                                      # 32-row tiles, two per frame
    Case("mfma_one_tile_3x4x64", "first", F=3, h=4, w=64),
    Case("mfma_frames2-5of7_16x16", "first", F=7, h=16, w=16, frames=(2, 5)),
    Case("generic_frames2-5of7_8x40", "first", F=7, h=8, w=40, frames=(2, 5)),
    Case("generic_Co16_3x8x12", "first", F=3, h=8, w=12, Co=16),
    Case("generic_Co96_2x6x10", "first", F=2, h=6, w=10, Co=96),
    Case("generic_Co16_4x256x256", "first", F=4, h=256, w=256, Co=16),                    # 4096 x 256 threads: the last grid without a second trip
    Case("generic_stride_7x236x40", "first", F=7, h=236, w=40),                           # 1,057,280 threads
    # ---- head_out
    *[Case(f"Co{Co}_r1003_{which}", "head", Co=Co, rows=1003, which=which) for Co in (128, 256) for which in ("both", "g", "o")],
]
