"""Shared by tools/gen_goldens_clip.py (build container, runs the reference sampler in every x0 clipping mode) and the tests that
consume tests/golden/clip_*.npz.  Inputs are those of ddim_tiny.npz (tiny cases) / fullsize_cases.build_inputs (C1); the per-step
noise is re-drawn from a seed instead of being stored, except for the S = 3 runs, which use the three tensors ddim_tiny.npz holds."""
import torch

CLIP_NOISE_SEED = 2468
KIND_CODES = {"dynamic": 0, "static": 1, "none": 2}          # = DAWN_CLIP_DYNAMIC / _STATIC / _NONE

# name -> (sampler, clipping mode as sampler.clip_mode takes it, cond_scale)
TINY_CASES = {
    "ddim_static": ("ddim", ("static",), 1.0),
    "ddim_static_guided": ("ddim", ("static",), 2.5),
    "ddim_none": ("ddim", ("none",), 1.0),
    "ddim_q50": ("ddim", ("dynamic", 0.5), 1.0),
    "ddim_q99": ("ddim", ("dynamic", 0.99), 1.0),
    "ddim_q100": ("ddim", ("dynamic", 1.0), 1.0),
    "ancestral_static": ("ancestral", ("static",), 1.0),
    "ancestral_q50_guided": ("ancestral", ("dynamic", 0.5), 2.5),
}
DDIM_S = (3, 50)                       # the S of ddim_tiny.npz and the benchmark's step count
# Without clipping nothing bounds the tiny model's latent: the reference's own sample reaches |x| = 19 after 3 steps and 404 after 50,
# where the parity gate (1e-4 max-abs) is under two fp32 ulps of the values.  The unclipped case therefore runs ddim_tiny's S only.
NONE_S = (3,)


def ddim_steps(name):
    return NONE_S if TINY_CASES[name][1][0] == "none" else DDIM_S


DDIM_KEEP = {3: (1, 2), 50: (1, 25, 49)}     # steps whose INPUT latent the fixtures keep
C1 = dict(T=16, h=32, S=50, keep=(25,))      # full architecture, DDIM, static; noise = fullsize_cases.ddim_noises(T, h, S)

PARITY_GATE = 1e-4                     # max-abs gate of the sampler parity tests (test_ancestral_cpu.TOL_X)
MODE_MARGIN = 100 * PARITY_GATE        # two modes must differ by more than this for a fixture to tell them apart


def ddim_noises_tiny(shape, S: int, tiny_noises=None, seed: int = CLIP_NOISE_SEED):
    """The S - 1 draws of torch.randn_like (MT:1201; none on the last step): ddim_tiny.npz's own tensors at its S = 3, one seeded
    CPU generator otherwise."""
    if S == 3 and tiny_noises is not None:
        return [torch.as_tensor(n) for n in tiny_noises][:S - 1]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g) for _ in range(S - 1)]
