"""Copy synthesis, wav -> ln-mel -> wav, with the m2s mel front end and HiFi-GAN generator (drop-in for inference.py).

Contract kept from the reference (inference.py:37-90): the flags ``--input_wavs_dir``, ``--output_dir``,
``--checkpoint_file``; ``config.json`` read from the checkpoint's directory; every file of the input directory
loaded with ``load_wav``, scaled by ``1 / MAX_WAV_VALUE``, turned into a mel with ``mel_spectrogram`` at the
config's ``n_fft / num_mels / sampling_rate / hop_size / win_size / fmin / fmax``; ``Generator(h)`` with
``ckpt['generator']`` loaded strictly; one ``{stem}_generated.wav`` per input at ``h.sampling_rate`` holding
``(audio * MAX_WAV_VALUE).astype(int16)`` (truncation).

Additive: ``--dtype`` (the generator's compute dtype) and ``--report FILE.json``, the round-trip mel L1 per file:
mean |mel(generated) - mel(input)|, the number train.py:228-252 validates with.  A file that cannot be read is
reported and skipped.  There is no CPU path.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from env import AttrDict  # noqa: E402
from meldataset import MAX_WAV_VALUE, load_wav, mel_spectrogram  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="wav -> ln-mel -> int16 wav (mel front end + HiFi-GAN generator on MI355X)")
    p.add_argument("--input_wavs_dir", default="test_files")
    p.add_argument("--output_dir", default="generated_files")
    p.add_argument("--checkpoint_file", required=True)
    p.add_argument("--dtype", choices=["bf16x3", "fp32", "bf16", "fp8"], default=None,
                   help="m2s compute dtype of the generator (default: M2S_DTYPE or bf16x3)")
    p.add_argument("--report", default=None, metavar="FILE.json",
                   help="write the round-trip mel L1 of every file (mean |mel(generated) - mel(input)|)")
    return p.parse_args(argv)


def get_mel(x, h):
    return mel_spectrogram(x, h.n_fft, h.num_mels, h.sampling_rate, h.hop_size, h.win_size, h.fmin, h.fmax)


def main(argv=None):
    from m2s import drivers

    args = parse_args(argv)
    ckpt = Path(args.checkpoint_file)
    h = AttrDict(json.loads((ckpt.parent / "config.json").read_text(encoding="utf-8")))
    if not torch.cuda.is_available():
        raise RuntimeError("m2s needs an MI355X (HIP) device; there is no CPU path")
    torch.manual_seed(h.seed)
    device = torch.device("cuda")
    gen, _ = drivers.build_generator(h, ckpt, device, args.dtype)

    src, out_dir = Path(args.input_wavs_dir), Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    from scipy.io.wavfile import write

    written, report = [], {}
    with torch.no_grad():
        for name in sorted(os.listdir(src)):
            try:
                data, _sr = load_wav(str(src / name))
                wav = torch.from_numpy(np.asarray(data, dtype=np.float32) / MAX_WAV_VALUE).to(device)
                if wav.dim() != 1:
                    raise ValueError(f"expected a mono file, got samples of shape {tuple(wav.shape)}")
                mel = get_mel(wav[None], h)
            except Exception as e:  # one bad file does not end the run
                print(f"[skip] {src / name}: {e}")
                continue
            audio = gen(mel).reshape(-1)
            path = out_dir / f"{Path(name).stem}_generated.wav"
            write(str(path), int(h.sampling_rate), drivers.int16_truncated(audio.cpu().numpy()))
            print(path)
            written.append(str(path))
            if args.report:
                back = get_mel(audio[None], h)
                t = min(int(back.shape[2]), int(mel.shape[2]))  # one frame fewer when n_fft - hop_size is odd
                report[name] = {"frames": int(mel.shape[2]), "samples": int(audio.numel()),
                                "mel_l1": float((back[:, :, :t] - mel[:, :, :t]).abs().mean())}
    if args.report:
        drivers.write_json(args.report, report)
    return written


if __name__ == "__main__":
    main()
