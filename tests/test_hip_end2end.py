"""-m gpu: the product path (Unet3D / GaussianDiffusion on HipOps) against the reference goldens and the
CPU oracle.  Tolerances (stated): predicted noise within 2e-5 abs of the reference golden on the tiny
config (values O(1); measured 2.3e-6 .. 5.6e-6); 1e-4 on the full DAWN_128 architecture (K up to 9216, ~300 chained ops,
fp32; measured 5.0e-6 .. 6.6e-6); trajectories 1e-5 (measured 1.2e-6)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, golden_sd
from oracle import dawn_oracle as O
import dawn_pytorch_amd as D
from dawn_pytorch_amd.policy import ConvPolicy

pytestmark = pytest.mark.gpu
T = torch.from_numpy
LOG = os.path.join(ROOT, "gpurun_out", "e2e_errors.jsonl")
TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3)


def log(name, got, want):
    err = float((got.cpu() - want.cpu()).abs().max())
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps({"case": name, "max_abs_err": err, "max_abs_ref": float(want.abs().max())}) + "\n")
    return err


def tiny_unet(sd):
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    return unet.cuda()


def test_loaded_native_library():
    from dawn_pytorch_amd import _lib
    assert _lib.lib().dawn_abi_version() == 8


def test_tiny_unet_golden(tiny):
    g, sd = tiny
    unet = tiny_unet(sd)
    y = unet.forward_with_cond_scale(T(g["x"]).cuda(), T(g["time"]).cuda(), cond=T(g["cond"]).cuda(), cond_scale=1.0)
    assert log("tiny_unet", y, T(g["y"])) < 2e-5
    y2 = unet.forward_with_cond_scale(T(g["x"]).cuda(), T(g["time"]).cuda(), cond=T(g["cond"]).cuda(), cond_scale=2.5)
    assert log("tiny_unet_cfg2.5", y2, T(g["y_cond_scale_2p5"])) < 5e-5
    h = load_golden("tiny_unet_T24.npz")
    unet.update_num_frames(24)
    y3 = unet.forward_with_cond_scale(T(h["x"]).cuda(), T(h["time"]).cuda(), cond=T(h["cond"]).cuda(), cond_scale=1.0)
    assert log("tiny_unet_T24", y3, T(h["y"])) < 2e-5


def test_long_clip_segmentation_of_the_unfused_attention_levels(tiny, monkeypatch):
    """The long-clip form of the unfused attention levels (qkv per frame segment, unet_forward.LONG_CLIP_FRAMES) on the HIP op set:
    == the whole-clip form and the reference golden (segment sizes shrunk so that the 24-frame golden runs several segments)."""
    from dawn_pytorch_amd import unet_forward as UF
    g, sd = tiny
    h = load_golden("tiny_unet_T24.npz")
    unet = tiny_unet(sd)
    unet.update_num_frames(24)
    args = (T(h["x"]).cuda(), T(h["time"]).cuda())
    whole = unet.forward_with_cond_scale(*args, cond=T(h["cond"]).cuda(), cond_scale=1.0)
    monkeypatch.setattr(UF, "LONG_CLIP_FRAMES", 4)
    monkeypatch.setattr(UF, "TEMPORAL_SEG_FRAMES", 9)          # 24 frames: 3 segments with win = 3 halo rows
    monkeypatch.setattr(UF, "FRAME_CHUNK", 7)
    seg = unet.forward_with_cond_scale(*args, cond=T(h["cond"]).cuda(), cond_scale=1.0)
    assert log("tiny_unet_T24_long_clip_segments_vs_whole", seg, whole.cpu()) < 5e-6
    assert log("tiny_unet_T24_long_clip_segments", seg, T(h["y"])) < 2e-5


def test_tiny_ddim_golden(tiny):
    g, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=12, denoise_fn=unet, num_frames=12, image_size=8,
                                        sampling_timesteps=int(d["S"]), timesteps=1000, loss_type='l2',
                                        use_dynamic_thres=True, null_cond_prob=0.1, ddim_sampling_eta=1.0).cuda()
    diff.update_num_frames(12)
    out = diff.sample(T(d["fea"]).cuda(), T(d["bbox"]).cuda(), cond=T(d["cond"]).cuda(), cond_scale=1.0,
                      x_init=T(d["x_init"]).cuda(), noises=[n.cuda() for n in T(d["noises"])], trace=True)
    qs = torch.stack([tr["s"][1] for tr in diff.last_trace[0]]).cpu()
    assert float((qs - T(d["quantiles"]).float()).abs().max()) < 5e-5
    assert log("tiny_ddim", out, T(d["out"])) < 1e-5


@pytest.mark.parametrize("Tn", [8, 5])
def test_full_dawn128_forward_vs_oracle(Tn):
    """Full DAWN_128 architecture (49.9 M params), h=32: HIP vs the CPU oracle.  T=8 runs the split-operand / LDS-halo
    kernels at every level; T=5 (odd) makes the deeper levels fall back to the other tile geometries / kernels."""
    h = 32
    unet = D.DynamicNfUnet3D(default_num_frames=Tn, dim=64, cond_dim=1032, cond_aud=1024, cond_pose=6, cond_eye=2,
                             num_frames=Tn, channels=275, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2, 4, 8),
                             use_hubert_audio_cond=True, learn_null_cond=False, use_final_activation=False,
                             use_deconv=True, padding_mode="zeros", win_width=40, init_seed=0)
    assert sum(p.numel() for p in set(unet.parameters())) == 49857555
    sd = {"denoise_fn." + k: v for k, v in unet.state_dict().items()}
    g = torch.Generator().manual_seed(123)
    fea = torch.randn(1, 272, h, h, generator=g)
    cond = torch.randn(1, Tn, 1032, generator=g)
    x3 = torch.randn(1, 3, Tn, h, h, generator=g)
    xin = torch.cat((x3, fea.unsqueeze(2).expand(-1, -1, Tn, -1, -1)), 1)
    want = O.unet_forward(sd, xin, torch.tensor([627]), cond, win=40)
    unet = unet.cuda()
    got = unet.forward_with_cond_scale(xin.cuda(), torch.tensor([627]).cuda(), cond=cond.cuda(), cond_scale=1.0)
    assert log(f"dawn128_T{Tn}_forward", got, want) < 1e-4


def test_sampler_properties_large():
    """Size-independent properties at a larger size: determinism of the Philox path and |x| <= clamp bound
    after the last step (alpha_next = 1 => x = clamp(x0)/s in [-1, 1])."""
    Tn, h = 48, 16
    unet = D.DynamicNfUnet3D(default_num_frames=Tn, dim=32, cond_dim=40, cond_aud=32, cond_pose=6, cond_eye=2,
                             num_frames=Tn, channels=35, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2, 4),
                             use_hubert_audio_cond=True, win_width=10).cuda()
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=Tn, denoise_fn=unet, num_frames=Tn, image_size=h,
                                        sampling_timesteps=4, timesteps=1000, loss_type='l2', use_dynamic_thres=True,
                                        ddim_sampling_eta=1.0).cuda()
    diff.noise_seed = 1234
    g = torch.Generator().manual_seed(5)
    fea, bbox = torch.randn(1, 28, h, h, generator=g).cuda(), torch.randn(1, 4, h, h, generator=g).cuda()
    cond = torch.randn(1, Tn, 40, generator=g).cuda()
    a = diff.sample(fea, bbox, cond=cond, cond_scale=1.0)
    b = diff.sample(fea, bbox, cond=cond, cond_scale=1.0)
    assert torch.equal(a, b), "sampler is not deterministic for a fixed Philox seed"
    assert torch.isfinite(a).all() and float(a.abs().max()) <= 1.0 + 1e-6


class _LoopbackComm:
    """World-size-1 stand-in for tshard.TShardComm: exercises the sharded code paths of HipOps (separate GroupNorm
    reduce / finalize kernels, histogram + min 'all-reduces', halo plumbing) without a second GPU."""
    Ttotal, f0 = 12, 0

    def all_reduce_sum(self, t):
        pass

    def all_reduce_min(self, t):
        pass

    def halo_exchange(self, x, HW, win):
        return x, 0

    def halo_begin(self, x, HW, win):
        from dawn_pytorch_amd.tshard import HaloExchange
        return HaloExchange(x, 0, 0, x.shape[0] // HW, [])

    def halo_end(self, hx):
        pass


def test_sharded_code_paths_world1(tiny):
    g, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=12, denoise_fn=unet, num_frames=12, image_size=8,
                                        sampling_timesteps=int(d["S"]), timesteps=1000, loss_type='l2',
                                        use_dynamic_thres=True, null_cond_prob=0.1, ddim_sampling_eta=1.0).cuda()
    out = diff.sample(T(d["fea"]).cuda(), T(d["bbox"]).cuda(), cond=T(d["cond"]).cuda(), cond_scale=1.0,
                      x_init=T(d["x_init"]).cuda(), noises=[n.cuda() for n in T(d["noises"])], comm=_LoopbackComm())
    assert log("tiny_ddim_sharded_paths", out, T(d["out"])) < 1e-5


def test_graph_replay_equals_eager():
    """HIP-graph replay of the UNet evaluation launches the same kernels as the eager path: bit-identical output."""
    Tn, h = 40, 16
    unet = D.DynamicNfUnet3D(default_num_frames=Tn, dim=64, cond_dim=40, cond_aud=32, cond_pose=6, cond_eye=2,
                             num_frames=Tn, channels=35, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2, 4),
                             use_hubert_audio_cond=True, win_width=10).cuda()
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=Tn, denoise_fn=unet, num_frames=Tn, image_size=h,
                                        sampling_timesteps=4, timesteps=1000, loss_type='l2', use_dynamic_thres=True,
                                        ddim_sampling_eta=1.0).cuda()
    diff.noise_seed = 99
    g = torch.Generator().manual_seed(5)
    fea, bbox = torch.randn(1, 28, h, h, generator=g).cuda(), torch.randn(1, 4, h, h, generator=g).cuda()
    cond = torch.randn(1, Tn, 40, generator=g).cuda()
    eager = diff.sample(fea, bbox, cond=cond, cond_scale=1.0)
    diff.use_graph = True
    graphed = diff.sample(fea, bbox, cond=cond, cond_scale=1.0)
    assert unet._ops().graph_error is None, unet._ops().graph_error
    assert torch.equal(eager, graphed)


@pytest.mark.parametrize("Tn,res", [(200, 256)])
def test_benchmark_size_kernel_families_agree(Tn, res):
    """At BASELINE's full size (256x256, 200 frames, DAWN_256 architecture) the CPU oracle takes minutes, so parity is
    checked through a size-independent property: one denoiser evaluation computed with the shipped kernel policy
    (split-operand bf16-pipe convs / GEMMs, LayerNorm in the GEMM loader, 256x64 / 256x128 tile policy, XCD remap) must
    agree with the same evaluation on the exact-fp32-MFMA kernels (ConvPolicy.EXACT_FP32: a different kernel family for every
    conv and projection; both families are checked against the oracle at small sizes).  Tolerance: 3e-5 x max|y| (measured 3.9e-6) --
    ~300 chained fp32 ops whose summation orders differ."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    from dawn_pytorch_amd.unet_forward import unet_forward
    dev = torch.device("cuda", 0)
    h = res // 4
    unet, _ = bench.build_model(Tn, h, 50, dev)
    fea, bbox, cond = bench.synthetic_inputs(Tn, h, dev)
    ops = unet._ops()
    P = unet.packed()
    cs = unet.build_clip(torch.cat((fea, bbox), 1)[0].contiguous(), cond[0].contiguous())
    x = torch.randn(3, Tn, h, h, generator=torch.Generator().manual_seed(9)).to(dev)
    try:
        y_split = unet_forward(ops, P, cs, x, 500)
        ops.conv_policy = ConvPolicy.EXACT_FP32
        y_fp32 = unet_forward(ops, P, cs, x, 500)
    finally:
        ops.conv_policy = 0                       # shipped policy
    torch.cuda.synchronize()
    assert torch.isfinite(y_split).all() and torch.isfinite(y_fp32).all()
    scale = float(y_fp32.abs().max())
    err = log(f"benchmark_size_T{Tn}_{res}px_split_vs_fp32_kernels", y_split, y_fp32)
    assert err <= 3e-5 * max(1.0, scale), (err, scale)
    # determinism of the shipped path at this size (no atomics in any reduction)
    assert torch.equal(unet_forward(ops, P, cs, x, 500), y_split)


def test_tshard_rccl_world1_equals_unsharded():
    """The T-shard path on the GPU over a real RCCL communicator (world size 1: the only size a 1-GPU box offers):
    `TShardComm` + the sharded orchestration (interior-first fused segments, separate GroupNorm reduce / all-reduce /
    finalize, histogram all-reduces) on a 64-channel model must reproduce the unsharded sampler.  Multi-rank equality
    is covered on CPU (tests/test_tshard_cpu.py, gloo, world 2-4)."""
    import socket
    import torch.distributed as dist
    from dawn_pytorch_amd.tshard import TShardComm
    Tn, h = 40, 16
    unet = D.DynamicNfUnet3D(default_num_frames=Tn, dim=64, cond_dim=40, cond_aud=32, cond_pose=6, cond_eye=2,
                             num_frames=Tn, channels=35, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2, 4),
                             use_hubert_audio_cond=True, win_width=10).cuda()
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=Tn, denoise_fn=unet, num_frames=Tn, image_size=h,
                                        sampling_timesteps=3, timesteps=1000, loss_type='l2', use_dynamic_thres=True,
                                        ddim_sampling_eta=1.0).cuda()
    diff.noise_seed = 5
    g = torch.Generator().manual_seed(5)
    fea, bbox = torch.randn(1, 28, h, h, generator=g).cuda(), torch.randn(1, 4, h, h, generator=g).cuda()
    cond = torch.randn(1, Tn, 40, generator=g).cuda()
    want = diff.sample(fea, bbox, cond=cond, cond_scale=1.0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    try:
        comm = TShardComm(dist, 0, 1, Tn, 0, Tn)
        got = diff.sample(fea, bbox, cond=cond, cond_scale=1.0, comm=comm)
        torch.cuda.synchronize()
        st = comm.stats()
    finally:
        if created:
            dist.destroy_process_group()
    assert st["all_reduces"] > 0 and st["halo_exchanges"] > 0 and st["halo_bytes_sent"] == 0
    assert log("tshard_rccl_world1_vs_unsharded", got, want) < 2e-5


def test_video_generator_pipeline_on_gpu(tmp_path):
    """The CLI contract end to end on the GPU (UVG:402-414) with every stage this build owns running on the HIP kernels:
    stage 2 `process_audio` (HuBERT features + 25 fps interpolation) -> stage 4 `generate_final_video`
    (FlowDiffusion.sample_one_video: DDIM sampler + UNet, LFG flow decode N1, frame egress N2).  Random-init weights of the
    shipped architectures (1024-wide HuBERT of reduced depth; full DAWN UNet; full LFG generator); the stages that are
    outside this build (3DDFA pose, PBnet) hand over through the cache files exactly as in the reference."""
    import argparse
    import sys
    import wave
    from PIL import Image
    from transformers import HubertConfig, HubertModel          # test infrastructure: supplies a reference-format state_dict
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.hubert import HubertFeatures
    from dawn_pytorch_amd.video_generator import VideoGenerator
    res, secs = 128, 2.6
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    hub_model = HubertModel(HubertConfig(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=512,
                                         conv_dim=(32,) * 7, conv_bias=True, feat_extract_norm="layer", do_stable_layer_norm=True,
                                         num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)).eval()
    hub = HubertFeatures.from_model(hub_model, "cuda:0")
    n = int(16000 * secs)
    pcm = (np.sin(np.arange(n) * 0.05) * 9000 + rng.standard_normal(n) * 800).astype("<i2")
    wav = tmp_path / "a.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm.tobytes())
    Tn = int(n / 16000 * 25)
    cache, outd = tmp_path / "cache", tmp_path / "out"
    cache.mkdir()
    np.save(cache / "dri_pose.npy", rng.standard_normal((Tn, 6)).astype(np.float32))      # PBnet stage output (out of scope)
    np.save(cache / "dri_blink.npy", rng.random((Tn, 2)).astype(np.float32))
    img = tmp_path / "face.png"
    Image.fromarray((rng.random((150, 150, 3)) * 255).astype(np.uint8)).save(img)
    cfg = {"input_size": res, "max_n_frames": 200, "random_seed": 1234, "mean": [0.0, 0.0, 0.0], "win_width": 40,
           "sampling_step": 3, "ddim_sampling_eta": 1.0, "cond_scale": 1.0, "model_config": {"is_train": True, "pose_dim": 6}}
    args = argparse.Namespace(audio_path=str(wav), image_path=str(img), output_path=str(outd), cache_path=str(cache), resolution=res)
    dec = FlowDecoder(bench_decode.lfg_state_dict(0), "cuda:0")
    vg = VideoGenerator(args, generator=dec, config=cfg, device="cuda:0", allow_random_weights=True, hubert=hub)
    frames = vg.run()
    feats = np.load(cache / "target_audio.npy")
    assert feats.shape == (Tn, 1024) and feats.dtype == np.float32 and np.isfinite(feats).all()
    assert frames.shape == (Tn, res, res, 3) and frames.dtype == np.uint8
    assert len(os.listdir(outd / "face" / "img")) == Tn
    out = vg.last_output
    assert out["sample_vid_grid"].shape == (1, 2, Tn, res // 4, res // 4) and torch.isfinite(out["sample_out_vid"]).all()
    # deterministic: the config's random_seed drives the counter-based noise
    vg2 = VideoGenerator(args, generator=dec, config=cfg, device="cuda:0", allow_random_weights=True, hubert=hub)
    vg2.video_model.load_state_dict(vg.video_model.state_dict())
    assert np.array_equal(vg2.run(), frames)


def test_tshard_rank_paths_agree_at_benchmark_length():
    """One interior T-shard rank's workload (tshard.SimulatedInteriorShard: 200 own frames + 2 x 40 halo frames, full DAWN
    architecture, 32 x 32 latent -- large enough for unet_forward._edge_first to take its early-post branch on the level-0 layers;
    at 8 x 8 both settings ran the same interior-first code): the edge-first schedule (producer writes the edge frames into
    comm.own_view, posts the exchange, computes the interior; the fused temporal layers then run as two balanced 100-query launches on
    the 280-row buffer) == the interior-first schedule (exchange posted by the temporal layer, 120 interior queries first, two 40-query
    edge launches): same arithmetic per query, so the two evaluations agree to fp32 rounding.  (Sharded == UNSHARDED is the business of
    tests/test_hip_shard_fullsize.py -- 8 in-process ranks at configs[3]'s full size -- and of tests/test_tshard_cpu.py over gloo.)"""
    from fullsize_cases import KW, build_inputs
    from dawn_pytorch_amd.tshard import SimulatedInteriorShard
    from dawn_pytorch_amd.unet_forward import unet_forward
    Tn, h = 200, 32
    unet = D.DynamicNfUnet3D(default_num_frames=Tn, **KW, init_seed=0).cuda()
    ops, P = unet._ops(), unet.packed()
    fea272, cond, x3 = build_inputs(Tn, h)
    fea272, cond, x3 = fea272[0].cuda().contiguous(), cond[0].cuda().contiguous(), x3[0].cuda().contiguous()
    outs = {}
    for edge_first in (True, False):
        comm = SimulatedInteriorShard(Tn, world=8, rank=3)
        comm.edge_first = edge_first
        cs = unet.build_clip(fea272, cond, comm=comm, Ttotal=comm.Ttotal, f0=comm.f0)
        outs[edge_first] = unet_forward(ops.with_comm(comm), P, cs, x3, 500)
        assert comm.n_halo == 10
        # init layer + the level-0 down / up layers (64 channels at 32 x 32) post early; the 16 x 16 level-1 up layer does not
        assert comm.n_halo_edge_first == (3 if edge_first else 0), comm.n_halo_edge_first
    torch.cuda.synchronize()
    assert torch.isfinite(outs[True]).all()
    err = log("tshard_rank_edge_first_vs_interior_first", outs[True], outs[False])
    assert err <= 2e-5 * max(1.0, float(outs[False].abs().max())), err
