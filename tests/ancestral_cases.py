"""Shared by tools/gen_goldens_ancestral.py (build container, runs the reference's ancestral sampler) and the tests that consume
tests/golden/ancestral_*.npz: the per-step noise of the 1000-step ancestral loop is re-drawn from the seed stored in the fixture
instead of being stored (1000 latents per clip)."""
import torch

ANCESTRAL_STEPS = 1000
ANCESTRAL_NOISE_SEED = 4321
KEEP = (1, 500, 900, 999)          # steps whose INPUT latent the fixtures keep


def ancestral_noises(shape, timesteps: int = ANCESTRAL_STEPS, seed: int = ANCESTRAL_NOISE_SEED):
    """The `timesteps` draws of torch.randn_like in p_sample (MT:1118), t = timesteps-1 ... 0, from one seeded CPU generator.
    The reference draws one at t = 0 too (masked out there), so the list has `timesteps` entries; the last one is never used."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*shape, generator=g) for _ in range(timesteps)]
