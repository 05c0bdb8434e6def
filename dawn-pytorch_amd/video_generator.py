"""`VideoGenerator`: CLI contract of SURVEY.md §8b B1(iv) (UVG = unified_video_generator.py, UVG:39-124,
304-414, 504-531, 588-603).  Only stage 4 ("Generating final video", UVG:304-400) is this build's hot
path; stages 1-3 (3DDFA pose, HuBERT, PBnet) are upstream stages that hand over through `.npy` files in
`cache_path` exactly as the reference does (UVG:199-200, 247, 301-302).  They are out of scope here: pass a
`frontend` object exposing `extract_pose / process_audio / generate_pose_blink` (e.g. the reference's own
class) or pre-populate the cache.

    python -m dawn_pytorch_amd.video_generator --image_path face.jpg --cache_path cache/tmp --resolution 256
"""
from __future__ import annotations

import argparse
import os
import os.path as osp
import shlex
import shutil
import subprocess
from typing import Optional

import numpy as np
import torch
import yaml

from .flow_diffusion import FlowDiffusion


class _LastOutput(dict):
    """`VideoGenerator.last_output` after a streamed decode.  The streaming path never materialises the fp32 clips, so
    "sample_out_vid" / "sample_warped_vid" are not stored; `out[key]`, `key in out` and `out.get(key)` answer for them all the same, by
    running `VideoGenerator.decode_last_clips()` once and keeping its result.  `keys()` and iteration list what is stored."""
    LAZY = ("sample_out_vid", "sample_warped_vid")

    def __init__(self, out, decode):
        super().__init__(out)
        self._decode = decode

    def __missing__(self, key):
        if key not in self.LAZY:
            raise KeyError(key)
        self.update(self._decode())
        return dict.__getitem__(self, key)

    def __contains__(self, key):
        return key in self.LAZY or dict.__contains__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default


class VideoGenerator:
    image_via_c = False               # (class default: the opt-in of __init__'s keyword)
    audio_via_c = False               # (likewise)

    def __init__(self, args, *, generator=None, frontend=None, config: Optional[dict] = None, device=None,
                 allow_random_weights: bool = False, deterministic: bool = True, hubert=None, pbnet=None,
                 video_egress: str = "png", encoder_cmd=None, pbnet_via_c: bool = False, inputs_via_c: bool = False,
                 image_via_c: bool = False, audio_via_c: bool = False):
        """`allow_random_weights`: explicit opt-in (benches, tests) to run with the deterministic random-init denoiser
        when the configured checkpoint is absent; without it a missing checkpoint raises, as the reference's
        `torch.load` does (UVG:527).  `deterministic`: seed the sampler's counter-based noise with the config's
        `random_seed` (the reference never seeds torch); False draws from torch's global generator.
        NOTE (reference quirk, kept): `FlowDiffusion.face_loc_emb` is never saved / loaded by the reference (it is a
        sibling of `.diffusion`, FD:169), so it stays at its constructor initialisation here too.
        `video_egress`: "png" = the reference's path (PNG files, then ffmpeg reads them back); "yuv420p" (native decode only) = the
        decoder writes planar YUV 4:2:0 frames, which stream into an encoder process's stdin chunk by chunk, and no PNG is written.
        `encoder_cmd` (yuv420p only): the encoder's argv (list, or a string split like a shell would), to which the output path
        `<output>/<name>/video/<name>.mp4` is appended; it reads raw I420 frames of the clip's size at 25 fps from stdin.  None: ffmpeg
        when there is one on PATH, else the frames go to `<name>.y4m` in the same directory.
        `pbnet_via_c`: stage 3 through the C-side stage (dawn_pose_blink_stage: windowed attention, any clip length) instead of the Python
        orchestration of pbnet.py.
        `inputs_via_c`: passed on as `FlowDiffusion.inputs_via_c` -- the face-location channels and the condition rows of a GPU clip from
        the C-side clip-input stage (dawn_clip_inputs) instead of the torch plumbing.
        `image_via_c` (GPU only): the decoded source image goes to the device as bytes and dawn_image_ingest resizes and scales it there
        (Pillow's 8-bit bilinear resample restated in integers: the same bytes as the host resize, and from there the same
        arithmetic as the default path, so the same frames); with `hubert` set, a 16 kHz 16-bit
        PCM file's frames go to the device as int16 and dawn_pcm16_to_samples makes the fp32 samples (the same values).
        `audio_via_c`: with `hubert` set, a 16-bit PCM WAV of any sample rate from 1000 to 384000 Hz never touches ffmpeg: on the GPU its
        frames go to the device as int16 and dawn_resample16k_pcm16 makes the 16 kHz samples, on a CPU device audio.resample_to_16k does
        (the same definition in numpy fp64).  The values are that definition's (include/dawn_hip.h), not ffmpeg's; nobody has measured
        the difference at the HuBERT features.  Any other file takes the default path."""
        if video_egress not in ("png", "yuv420p"):
            raise ValueError(f"video_egress must be 'png' or 'yuv420p', not {video_egress!r}")
        self.video_egress = video_egress
        self.encoder_cmd = shlex.split(encoder_cmd) if isinstance(encoder_cmd, str) else (list(encoder_cmd) if encoder_cmd else None)
        self.hubert = hubert              # hubert.HubertFeatures: stage 2 (process_audio, UVG:202-250) on the GPU
        self.pbnet_via_c = bool(pbnet_via_c)
        self.inputs_via_c = bool(inputs_via_c)
        self.image_via_c = bool(image_via_c)
        self.audio_via_c = bool(audio_via_c)
        self.pbnet = pbnet               # (pose, blink) pbnet.PoseBlinkGenerator pair: stage 3 (generate_pose_blink, UVG:252-302; N4)
        self.allow_random_weights = bool(allow_random_weights) or bool(getattr(args, "allow_random_weights", False))
        self.deterministic = deterministic
        self.audio_path = args.audio_path
        self.image_path = args.image_path
        self.output_path = args.output_path
        self.cache_path = args.cache_path
        self.resolution = args.resolution
        self.frontend = frontend
        self.device = torch.device(device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
        os.makedirs(self.cache_path, exist_ok=True)
        os.makedirs(self.output_path, exist_ok=True)
        self.audio_emb_path = os.path.join(self.cache_path, 'target_audio.npy')
        if config is None:
            cfg_path = getattr(args, "config", None) or osp.join('config', f'DAWN_{int(self.resolution)}.yaml')
            with open(cfg_path) as f:
                config = yaml.safe_load(f)
        self.video_config = config
        for k in ("sampling_step", "max_n_frames"):                  # BASELINE overrides (50 steps, long clips)
            v = getattr(args, k, None)
            if v is not None:
                self.video_config[k] = v
        self.video_model = self._init_video_model(self.video_config['model_config'], generator)

    def _init_video_model(self, model_config, generator=None):
        """UVG:504-531."""
        model = FlowDiffusion(is_train=model_config['is_train'], sampling_timesteps=self.video_config['sampling_step'],
                              ddim_sampling_eta=self.video_config['ddim_sampling_eta'],
                              pose_dim=model_config['pose_dim'], config_pth=model_config.get('config_pth'),
                              pretrained_pth=model_config.get('ae_pretrained_pth'),
                              win_width=self.video_config['win_width'], generator=generator, device=self.device)
        model.to(self.device)
        ckpt_path = model_config.get('diffusion_pretrained_pth')
        if ckpt_path and osp.exists(ckpt_path):
            checkpoint = torch.load(ckpt_path, map_location=self.device)
            model.diffusion.load_state_dict(checkpoint['diffusion'])          # UVG:527-528, 912 keys, strict
        elif not self.allow_random_weights:
            raise FileNotFoundError(
                f"diffusion checkpoint {ckpt_path!r} (model_config.diffusion_pretrained_pth) not found; sampling with "
                "random-init weights would silently write a garbage video.  Pass allow_random_weights=True "
                "(--allow_random_weights) to do that on purpose (benches / plumbing tests).")
        seed = self.video_config.get('random_seed')
        if seed is not None and self.deterministic:
            model.diffusion.noise_seed = int(seed)   # the reference never seeds torch; we can
        model.inputs_via_c = self.inputs_via_c
        model.eval()
        return model

    # ---- upstream stages: delegated
    def extract_pose(self):
        return self._front("extract_pose")

    def process_audio(self):
        """UVG:202-250.  With a `hubert.HubertFeatures` object (built from the reference's own HubertModel state_dict) the
        stage runs here: 16 kHz waveform -> HuBERT hidden states (chunked as UVG:466-501) -> 25 fps linear interpolation ->
        `target_audio.npy`.  Otherwise it is delegated to `frontend` / the cache like the other upstream stages."""
        if self.hubert is None or not (self.audio_path and osp.exists(self.audio_path)):
            return self._front("process_audio")
        any_rate = self._pcm_any_rate() if self.audio_via_c else None
        pcm = read_pcm16_16k(self.audio_path) if any_rate is None and self.image_via_c and self.device.type == "cuda" else None
        if any_rate is not None:
            frames, rate = any_rate
            if self.device.type == "cuda":
                speech = self.video_model.unet._ops().resample_to_16k(torch.from_numpy(frames).to(self.device), rate)
            else:
                from .audio import resample_to_16k
                speech = resample_to_16k(frames, rate)
        elif pcm is not None:
            speech = self.video_model.unet._ops().pcm16_to_samples(torch.from_numpy(pcm).to(self.device))
        else:
            speech = load_wav_16k(self.audio_path)
        feats = self.hubert.process_audio(speech)
        print(f'Frame count: {feats.shape[0]}')
        np.save(self.audio_emb_path, feats)

    def _pcm_any_rate(self):
        """(int16 frames (n, channels), rate) of the audio file where `audio_via_c` takes it -- 16-bit PCM, a rate the resampler takes, at
        least one 16 kHz sample -- else None."""
        from .audio import MAX_RATE, MIN_RATE, read_pcm16, resample_len
        got = read_pcm16(self.audio_path)
        if got is None or not MIN_RATE <= got[1] <= MAX_RATE or resample_len(got[0].shape[0], got[1]) < 1:
            return None
        return got

    def generate_pose_blink(self):
        """UVG:252-302.  With a (pose, blink) pair of `pbnet.PoseBlinkGenerator` (built from the decoders of the reference's own
        PBnet checkpoints) the stage runs here: init_pose.npy / init_eye_bbox.npy (or the reference's defaults when the 3DDFA
        extraction left none, UVG:275-279) + target_audio.npy -> dri_pose.npy / dri_blink.npy.  Otherwise delegated."""
        if self.pbnet is None:
            return self._front("generate_pose_blink")
        from .pbnet import pose_blink_stage
        try:
            init_pose = torch.from_numpy(np.load(osp.join(self.cache_path, 'init_pose.npy')))
            init_blink = torch.from_numpy(np.load(osp.join(self.cache_path, 'init_eye_bbox.npy')))
        except Exception:                                     # noqa: BLE001  (UVG:275: default values when 3DDFA extraction failed)
            init_pose = torch.from_numpy(np.array([[0, 0, 0, 4.79e-04, 5.65e+01, 6.49e+01]]))
            init_blink = torch.from_numpy(np.array([[0.3, 0.3]]))
        audio = torch.from_numpy(np.load(self.audio_emb_path))
        pose, blink = pose_blink_stage(self.pbnet[0], self.pbnet[1], audio, init_pose, init_blink, via_c=self.pbnet_via_c)
        np.save(osp.join(self.cache_path, 'dri_pose.npy'), pose.numpy())
        np.save(osp.join(self.cache_path, 'dri_blink.npy'), blink.numpy())

    def _front(self, name):
        if self.frontend is not None:
            return getattr(self.frontend, name)()
        need = {"extract_pose": ['init_pose.npy', 'init_eye_bbox.npy'], "process_audio": ['target_audio.npy'],
                "generate_pose_blink": ['dri_pose.npy', 'dri_blink.npy']}[name]
        missing = [f for f in need if not osp.exists(osp.join(self.cache_path, f))]
        if missing and name != "extract_pose":      # extract_pose has defaults in the reference (UVG:335-341)
            raise RuntimeError(f"stage '{name}' is outside this build (SURVEY §2 #11-13): provide a `frontend` or the "
                               f"cache files {missing} in {self.cache_path}")

    def generate_final_video(self):
        """UVG:304-400."""
        from PIL import Image
        cfg = self.video_config
        name = os.path.splitext(os.path.basename(self.image_path))[0]
        video_dir = os.path.join(self.output_path, name, 'video')
        img_dir = os.path.join(self.output_path, name, 'img')
        yuv = self.video_egress == "yuv420p"
        os.makedirs(video_dir, exist_ok=True)
        if not yuv:
            os.makedirs(img_dir, exist_ok=True)
        size = cfg['input_size']
        image = Image.open(self.image_path).convert("RGB")
        if self.image_via_c and self.device.type == "cuda":
            # the decoded bytes as they are; resize, planes and ToTensor() on the device (dawn_image_ingest), then the reference's * 255
            # (UVG:325): byte / 255 * 255 is the byte again for all 256 values, so this is the tensor of the branch below, bit for bit
            planes = self.video_model.unet._ops().image_ingest(torch.from_numpy(np.array(image)).to(self.device), size, size)
            image_tensor = planes * 255
        else:
            image = image.resize((size, size), Image.BILINEAR)
            image_tensor = torch.from_numpy(np.array(image)).permute(2, 0, 1).float()    # 0..255, like ToTensor()*255
        hubert = np.load(self.audio_emb_path)
        T = min(cfg['max_n_frames'], hubert.shape[0])
        ref_hubert = torch.from_numpy(hubert[:T]).float()
        poses = torch.from_numpy(np.load(osp.join(self.cache_path, 'dri_pose.npy'))[:T]).float()
        blink = torch.from_numpy(np.load(osp.join(self.cache_path, 'dri_blink.npy'))[:T]).float()
        try:
            real_poses = torch.from_numpy(np.load(osp.join(self.cache_path, 'init_pose.npy'))).float()
            real_bb = torch.from_numpy(np.load(osp.join(self.cache_path, 'init_eye_bbox.npy'))).float()
        except Exception:
            real_poses = torch.zeros(1, 7)                                                  # UVG:338-341 defaults
            real_bb = torch.tensor([[0.3, 0.3, 64, 64, 192, 192, 256, 256]]).reshape(1, -1).float()
        init_pose = real_poses[0].unsqueeze(0)
        init_blink = real_bb[0, :2].unsqueeze(0)
        poses, blink, real_bb = poses.permute(1, 0), blink.permute(1, 0), real_bb.permute(1, 0)
        dev = self.device
        mean = tuple(cfg.get('mean', (0, 0, 0)))
        sample_img = image_tensor.unsqueeze(0).to(dev) / 255.
        stream = self.video_model.decodes_natively(sample_img)
        if yuv and not stream:
            raise ValueError("video_egress='yuv420p' needs the native flow decode (native_decode, or a clip on the GPU)")
        egress = dict(format="yuv420p", mean=mean, stream=True) if yuv else dict(mean=mean, bgr=False, stream=True)
        with torch.no_grad():
            self.video_model.update_num_frames(T)
            out = self.video_model.sample_one_video(
                sample_img=sample_img, sample_audio_hubert=ref_hubert.unsqueeze(0).to(dev),
                sample_pose=poses.unsqueeze(0).to(dev), sample_eye=blink[:2].unsqueeze(0).to(dev),
                sample_bbox=real_bb[2:].unsqueeze(0).to(dev), init_pose=init_pose.to(dev), init_eye=init_blink.to(dev),
                cond_scale=cfg['cond_scale'], frames_u8=egress if stream else None)
        if yuv:
            # the decoder's last kernel writes what the encoder reads; each chunk goes to the encoder while the next one decodes
            frames = self._encode_yuv420(out.pop("sample_frames_yuv420"), T, size, size, video_dir, name)
            self._last_clip = (sample_img, out["sample_vid_grid"], out["sample_vid_conf"])
            self.last_output = _LastOutput(out, self.decode_last_clips)
            return frames
        # frame egress (UVG:383-397 + `_process_output_frame` UVG:533-548), RGB order here (PIL); `bgr=True` gives cv2's order.
        if stream:
            # native decode: the decoder's last kernel writes the (T,H,W,3) bytes itself (numpy's exact arithmetic), chunk by chunk;
            # each chunk's device->host copy and PNG encoding overlap the decode of the next one, and no fp32 clip is materialised
            frames = np.empty((T, size, size, 3), dtype=np.uint8)
            for t0, chunk in out.pop("sample_frames_u8"):
                frames[t0:t0 + len(chunk)] = chunk
                for i, fr in enumerate(chunk, start=t0):
                    Image.fromarray(fr).save(os.path.join(img_dir, f"{i:03d}.png"))
            self._last_clip = (sample_img, out["sample_vid_grid"], out["sample_vid_conf"])
            out = _LastOutput(out, self.decode_last_clips)
        else:
            # the injected generator decoded frame by frame: one conversion launch for the whole clip and ONE device->host copy
            frames = self.video_model.unet._ops().frames_to_u8(out["sample_out_vid"][0].float().contiguous(), mean=mean,
                                                               bgr=False).cpu().numpy()
            for i, fr in enumerate(frames):
                Image.fromarray(fr).save(os.path.join(img_dir, f"{i:03d}.png"))
        self.last_output = out
        mp4 = os.path.join(video_dir, f"{name}.mp4")
        try:                                                                                 # UVG:566-586 (ffmpeg mux)
            cmd = ['ffmpeg', '-y', '-framerate', '25', '-i', os.path.join(img_dir, '%03d.png')]
            if self.audio_path and osp.exists(self.audio_path):
                cmd += ['-i', self.audio_path, '-shortest']
            subprocess.run(cmd + ['-pix_fmt', 'yuv420p', mp4], check=False, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
        except FileNotFoundError:
            pass
        return frames

    def _yuv420_encoder(self, H: int, W: int, mp4: str):
        """argv of the process that reads the raw I420 stream from stdin and writes `mp4`, or None: no encoder here."""
        if self.encoder_cmd is not None:
            return self.encoder_cmd + [mp4]
        if shutil.which("ffmpeg") is None:
            return None
        cmd = ['ffmpeg', '-y', '-f', 'rawvideo', '-pix_fmt', 'yuv420p', '-s', f'{W}x{H}', '-framerate', '25',
               '-color_range', 'tv', '-colorspace', 'smpte170m', '-i', '-']                # BT.601 limited range, as the frames are
        if self.audio_path and osp.exists(self.audio_path):
            cmd += ['-i', self.audio_path, '-shortest']
        return cmd + ['-pix_fmt', 'yuv420p', mp4]

    def _encode_yuv420(self, chunks, T: int, H: int, W: int, video_dir: str, name: str) -> np.ndarray:
        """Feed the (t0, (n, 3HW/2) uint8) chunks of FlowDecoder.stream_frames_yuv420 to the encoder's stdin as they arrive -- or, with
        no encoder, to `<name>.y4m` -- and return all of them as one (T, 3HW/2) array.  The encoder is a child process (Popen); its
        stdin is closed and it is waited for; a non-zero exit or a broken pipe raises."""
        frames = np.empty((T, H * W * 3 // 2), dtype=np.uint8)
        cmd = self._yuv420_encoder(H, W, os.path.join(video_dir, f"{name}.mp4"))
        if cmd is None:
            with open(os.path.join(video_dir, f"{name}.y4m"), "wb") as f:
                f.write(f"YUV4MPEG2 W{W} H{H} F25:1 Ip A1:1 C420jpeg\n".encode())
                for t0, chunk in chunks:
                    frames[t0:t0 + len(chunk)] = chunk
                    for fr in chunk:
                        f.write(b"FRAME\n")
                        f.write(fr.tobytes())
            return frames
        proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        broken = None
        try:
            for t0, chunk in chunks:
                frames[t0:t0 + len(chunk)] = chunk
                proc.stdin.write(chunk.tobytes())
            proc.stdin.close()
        except BrokenPipeError as e:                                                        # the encoder went away mid-stream
            broken = e
        finally:
            if hasattr(chunks, "close"):
                chunks.close()
            if broken is not None or not proc.stdin.closed:
                try:
                    proc.stdin.close()
                except OSError:
                    pass
            rc = proc.wait()
        if broken is not None or rc != 0:
            raise RuntimeError(f"video encoder {cmd[0]!r} failed (exit status {rc}"
                               f"{', broken pipe' if broken is not None else ''})") from broken
        return frames

    def decode_last_clips(self):
        """The fp32 clips {"sample_out_vid", "sample_warped_vid"} (B,3,T,H,W) of the last streamed `generate_final_video`: that
        path writes bytes only, so they cost one more decode of the clip, run here on request (`last_output[...]` asks for it)."""
        img, grid, conf = self._last_clip
        return self.video_model.flow_decoder(img.device).decode_clip(img, grid, conf)

    def run(self):
        """UVG:402-414."""
        print("1. Extracting pose information...")
        self.extract_pose()
        print("2. Processing audio...")
        self.process_audio()
        print("3. Generating pose and blink data...")
        self.generate_pose_blink()
        print("4. Generating final video...")
        return self.generate_final_video()


def read_pcm16_16k(path: str) -> Optional[np.ndarray]:
    """The frames of a 16 kHz 16-bit PCM WAV as int16 (n_frames, channels), read with the stdlib; None for any other file."""
    import wave
    try:
        with wave.open(path, "rb") as f:
            sr, nch, sw, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
    except (wave.Error, EOFError):
        return None
    if sr != 16000 or sw != 2 or not 1 <= nch <= 8 or len(raw) < 2 * nch:
        return None
    return np.frombuffer(raw, dtype="<i2").reshape(-1, nch).copy()


def load_wav_16k(path: str) -> np.ndarray:
    """The reference converts with `ffmpeg -ar 16000` into a temp file and reads it with soundfile (UVG:220-227, 416-431):
    float64 samples in [-1, 1).  Host I/O only: a 16 kHz PCM WAV is read directly (stdlib `wave`); anything else goes
    through the same ffmpeg command first."""
    import tempfile
    import wave

    def read_pcm(p):
        with wave.open(p, "rb") as f:
            sr, nch, sw, n = f.getframerate(), f.getnchannels(), f.getsampwidth(), f.getnframes()
            raw = f.readframes(n)
        if sw != 2:
            raise ValueError(f"{p}: only 16-bit PCM WAV is read natively (sample width {sw})")
        x = np.frombuffer(raw, dtype="<i2").astype(np.float64) / 32768.0        # soundfile's int16 -> float64 scaling
        return (x.reshape(-1, nch) if nch > 1 else x), sr

    try:
        x, sr = read_pcm(path)
        if sr == 16000:
            return x
    except (wave.Error, ValueError):
        pass
    with tempfile.NamedTemporaryFile("w", suffix=".wav") as tmp:
        subprocess.run(["ffmpeg", "-i", path, "-ar", "16000", "-y", tmp.name], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        x, sr = read_pcm(tmp.name)
    if not (sr == 16000):
        raise ValueError("sr == 16000")
    return x


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--audio_path', type=str, default='WRA_MarcoRubio_000.wav')
    p.add_argument('--image_path', type=str, default='real_female_1.jpeg')
    p.add_argument('--output_path', type=str, default='output')
    p.add_argument('--cache_path', type=str, default='cache/tmp')
    p.add_argument('--resolution', type=int, default=128)
    p.add_argument('--config', type=str, default=None, help='DAWN_{res}.yaml (defaults to ./config/DAWN_<res>.yaml)')
    p.add_argument('--sampling_step', type=int, default=None, help='override the sampler steps (YAML ships 20): DDIM below 1000, '
                   'the 1000-step ancestral loop at 1000 or more')
    p.add_argument('--max_n_frames', type=int, default=None, help='override the clip-length cap (YAML ships 200)')
    p.add_argument('--pbnet_pose_ckpt', type=str, default='./pretrain_models/pbnet_seperate/pose/checkpoint_40000.pth.tar')
    p.add_argument('--pbnet_blink_ckpt', type=str, default='./pretrain_models/pbnet_seperate/blink/checkpoint_95000.pth.tar')
    p.add_argument('--video_egress', type=str, default='png', choices=('png', 'yuv420p'),
                   help='png: PNG frames that ffmpeg reads back (the reference); yuv420p: the decoder writes planar YUV 4:2:0, piped '
                        'into the encoder as it decodes (no PNG files)')
    p.add_argument('--allow_random_weights', action='store_true',
                   help='run with the deterministic random-init denoiser when the checkpoint is absent (plumbing only)')
    return p.parse_args(argv)


def main():
    args = parse_args()
    pbnet = None
    if osp.exists(args.pbnet_pose_ckpt) and osp.exists(args.pbnet_blink_ckpt):     # stage 3 here, else via the cache files
        from .pbnet import load_pbnet
        pbnet = load_pbnet(args.pbnet_pose_ckpt, args.pbnet_blink_ckpt, device="cuda:0" if torch.cuda.is_available() else "cpu")
    VideoGenerator(args, pbnet=pbnet, video_egress=args.video_egress).run()


if __name__ == "__main__":
    main()
