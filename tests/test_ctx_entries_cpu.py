"""Which C entry each CtxEvaluator sampler method reaches, and what it hands it -- without a device: the library is a recording
stand-in, the tensors live on the CPU.  (What the entries compute, and that they agree bit for bit, is the GPU tests' business.)"""
import itertools

import pytest
import torch

from dawn_pytorch_amd import _lib
from dawn_pytorch_amd import ctx as X
from dawn_pytorch_amd import sampler as SM

S, F, H, W = 6, 12, 8, 8
BUFS = SM.cosine_schedule_buffers()
STEPS = {"sample": SM.ddim_step_scalars(BUFS, S, 1.0),
         "sample_ancestral": SM.ancestral_step_scalars(SM.cosine_schedule_buffers(S), S),
         "sample_dpmpp": SM.dpmpp_step_scalars(BUFS, S)}
SOLVER = {"sample": (X.SOLVER_DDIM, X.DdimStep), "sample_ancestral": (X.SOLVER_ANCESTRAL, X.AncestralStep),
          "sample_dpmpp": (X.SOLVER_DPMPP, X.DpmppStep)}
# precedence left to right: known / known_entry, x0_clip given, guided, shard, neither
ENTRY = {"sample": ("dawn_sampler_run_known", "dawn_sampler_run_clip", "dawn_sampler_run_guided", "dawn_sampler_run_sharded",
                    "dawn_sampler_run"),
         "sample_ancestral": ("dawn_sampler_run_known", "dawn_sampler_run_ancestral_clip") + ("dawn_sampler_run_ancestral",) * 3,
         "sample_dpmpp": ("dawn_sampler_run_known",) + ("dawn_sampler_run_dpmpp",) * 4}
NO_NULL_CLIP = ("dawn_sampler_run", "dawn_sampler_run_sharded")      # (c, F, h, w, clip_mem, x_init, S, steps, ...)


class RecordingLib:
    """Every dawn_workspace_bytes* call answers a small size, every other entry 0 (success); `calls` keeps the latter."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            if name.startswith("dawn_workspace_bytes"):
                return 4096
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture()
def ev():
    e = X.CtxEvaluator.__new__(X.CtxEvaluator)
    e.L, e.device, e.h = RecordingLib(), "cpu", None
    e._need, e._policy, e._ws = {}, 0, None
    e._stream = lambda: 0
    return e


def _clip():
    return {"mem": torch.zeros(16, dtype=torch.uint8), "F": F, "h": H, "w": W}


def _shard():
    nop = lambda *a: None                                            # noqa: E731
    return X.ShardCallbacks(1, 2, nop, nop, nop, nop, nop)


@pytest.mark.parametrize("method", sorted(ENTRY))
@pytest.mark.parametrize("shard,guided,clipped,known_entry", list(itertools.product((False, True), repeat=4)))
def test_entry_table(ev, method, shard, guided, clipped, known_entry):
    steps = STEPS[method]
    kw = dict(shard=_shard() if shard else None, x0_clip=("static",) if clipped else None, known_entry=known_entry,
              want_thresholds=True)
    null_clip = None
    if guided:
        null_clip = _clip()
        kw.update(null_clip=null_clip, cond_scale=2.0)
    if method != "sample_dpmpp":
        kw["seed"] = 5
    out, thr = getattr(ev, method)(_clip(), torch.zeros(3, F, H, W), steps, **kw)
    assert out.shape == (3, F, H, W) and thr.shape == (S, 2)
    (name, args), = ev.L.calls
    want = ENTRY[method][0 if known_entry else 1 if clipped else 2 if guided else 3 if shard else 4]
    assert name == want
    assert len(args) == len(_lib.SIGNATURES[name])
    i_s = 6 if name in NO_NULL_CLIP else 8
    assert args[i_s] == S
    solver, step_type = SOLVER[method]
    if name == "dawn_sampler_run_known":
        assert args[i_s + 1] == solver
        arr = args[i_s + 2]
    else:
        arr = args[i_s + 1]
    assert arr._type_ is step_type and len(arr) == S
    if name not in NO_NULL_CLIP:                                     # null_clip_mem: only when guided
        assert args[5] == (null_clip["mem"].data_ptr() if guided else None)
        assert args[6] == (2.0 if guided else 1.0)
    for i, st in enumerate(steps):
        for field, ctype in step_type._fields_:
            assert getattr(arr[i], field) == ctype(st[field]).value, (i, field)


@pytest.mark.parametrize("method", ["sample", "sample_ancestral"])
def test_a_missing_noise_of_a_step_that_draws_is_refused(ev, method):
    """noises[i] = None where step i draws noise: the C loop would take it for "no noise" and return a wrong clip."""
    with pytest.raises(_lib.DawnHipError, match=rf"^{method}: noises\[0\] missing"):
        getattr(ev, method)(_clip(), torch.zeros(3, F, H, W), STEPS[method], noises=[None] * S)
    assert ev.L.calls == []
