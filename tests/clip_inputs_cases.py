"""Cases and CPU references of the clip-input kernels (csrc/clip_inputs.hip: dawn_face_loc_embed, dawn_cond_rows), shared by
tests/test_clip_inputs_cpu.py and tests/test_hip_clip_inputs.py.  The yardstick is code that predates the kernels, run on the CPU:
`FlowDiffusion.generate_bbox_mask` (the rectangle), `Face_loc_Encoder` (float64 = want64, float32 = base32) and
`FlowDiffusion.assemble_cond` (the condition rows: a single fp32 subtraction has one answer, so `torch.equal`)."""
import warnings

import torch

from dawn_pytorch_amd.flow_diffusion import Face_loc_Encoder, FlowDiffusion

# (name, size, bbox6 = [x_min, x_max, y_min, y_max, H_src, W_src]) -- what each reaches is stated in tests/test_hip_clip_inputs.py
BBOX_CASES = [
    ("fallback", 256, [64, 64, 192, 192, 256, 256]),
    ("odd_phase", 68, [37, 90, 21, 75, 256, 256]),
    ("even_phase", 68, [40, 96, 24, 80, 256, 256]),
    ("tile_edge", 64, [60, 130, 60, 130, 256, 256]),
    ("full_smallest", 8, [0, 255, 0, 255, 256, 256]),
    ("beyond", 36, [-20, 400, -3, 300, 256, 256]),
    ("empty", 36, [200, 100, 200, 100, 256, 256]),
    ("corner", 36, [250, 255, 250, 255, 256, 256]),
    ("non_square_source", 256, [300, 700, 200, 900, 720, 1080]),
]


class _Bare(FlowDiffusion):
    """FlowDiffusion's host-side methods without its UNet (generate_bbox_mask / assemble_cond read only `pose_dim`)."""

    def __init__(self, pose_dim):                    # noqa: super().__init__ builds the whole model; the two methods need none of it
        torch.nn.Module.__init__(self)
        self.pose_dim = pose_dim


def bare(pose_dim=7):
    return _Bare(pose_dim)


def mask_of(bbox6, size):
    """generate_bbox_mask for one sample -> (size, size) float mask."""
    b = torch.tensor(bbox6, dtype=torch.float32).view(1, 6, 1)
    return bare().generate_bbox_mask(b, size=size)[0, 0]


def mask_from_bounds(bounds, size):
    """The mask the four ints of dawn_bbox_mask_bounds describe (lt_x, lt_y, rb_x, rb_y)."""
    lt_x, lt_y, rb_x, rb_y = bounds
    r = torch.arange(size).view(size, 1)
    c = torch.arange(size).view(1, size)
    return ((r >= lt_y) & (r <= rb_y) & (c >= lt_x) & (c <= rb_x)).float()


def encoder_weights(seed=0):
    """Seeded N(0, 0.5) weights and biases: ReLU cuts about half the values (the default initialisation leaves almost everything near
    zero).  -> dict of the four state_dict tensors (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g) * 0.5                                        # noqa: E731
    return {"conv1.weight": r(8, 1, 3, 3), "conv1.bias": r(8), "conv2.weight": r(16, 8, 3, 3), "conv2.bias": r(16)}


_refs = {}


def encoder_refs(name, seed=0):
    """(want64, base32) of Face_loc_Encoder(generate_bbox_mask(bbox)) for a BBOX_CASES entry, each (16, size/4, size/4); computed once.
    base32 through torch's im2col + GEMM convolution, as split_gate.Case.base32."""
    key = (name, seed)
    if key not in _refs:
        _, size, bbox6 = next(c for c in BBOX_CASES if c[0] == name)
        m = mask_of(bbox6, size)[None, None]
        enc = Face_loc_Encoder()
        enc.load_state_dict(encoder_weights(seed))
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.backends.mkldnn.flags(enabled=False), torch.backends.nnpack.flags(enabled=False):
                base32 = enc(m)[0]
            want64 = enc.double()(m.double())[0]
        _refs[key] = (want64, base32)
    return _refs[key]


# ---------------------------------------------------------------------------------------------- condition rows
COND_T = [1, 3, 200, 1025]
# (n_pose, n_init): 0 = init_pose absent (row 0 of the pose stands in)
COND_POSE = [(6, 6), (6, 7), (6, 0), (7, 7)]
N_AUD = 1024


def cond_inputs(T, n_pose, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * T + n_pose)
    audio = torch.randn(T, N_AUD, generator=g)
    pose = torch.randn(T, n_pose, generator=g) * 20.0
    eye = torch.rand(T, 2, generator=g)
    return audio, pose, eye


def cond_inits(n_init, with_eye, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * n_init)
    ip = (torch.randn(n_init, generator=g) * 20.0).tolist() if n_init else None
    ie = torch.rand(2, generator=g).tolist() if with_eye else None
    return ip, ie


def cond_want(audio, pose, eye, init_pose, init_eye):
    """FlowDiffusion.assemble_cond for one sample on the CPU -> (T, n_aud + P + 2)."""
    P = len(init_pose) if init_pose is not None else pose.shape[1]
    fd = bare(P)
    ip = None if init_pose is None else torch.tensor(init_pose, dtype=torch.float32)[None]
    ie = None if init_eye is None else torch.tensor(init_eye, dtype=torch.float32)[None]
    return fd.assemble_cond(audio[None], pose.t()[None], eye.t()[None], ip, ie)[0]
