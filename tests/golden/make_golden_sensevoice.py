"""Writes tests/golden/sensevoice_fbank.npz: HF transformers' `audio_utils.spectrogram` with Kaldi settings
(an independent Kaldi-compatible fbank) for the deterministic audio the SenseVoice tests share.

    python tests/golden/make_golden_sensevoice.py

Per length n of sensevoice_torch.FIXTURE_LENGTHS (case index ci): `c{n}_frames` (the frame count) and
`c{n}_fbank` -- all frames for the short cases, the rows of fixture_rows(T) for the long ones, so the
file stays small."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import sensevoice_torch as ST  # noqa: E402


def fixture_rows(T):
    """the frames a fixture keeps: all up to 64, else the first 24, 16 around the middle and the last 24"""
    if T <= 64:
        return np.arange(T)
    return np.concatenate([np.arange(24), np.arange(T // 2 - 8, T // 2 + 8), np.arange(T - 24, T)])


def hf_fbank(pcm):
    from transformers.audio_utils import mel_filter_bank, spectrogram, window_function
    fb = mel_filter_bank(num_frequency_bins=257, num_mel_filters=80, min_frequency=20.0, max_frequency=8000.0,
                         sampling_rate=16000, norm=None, mel_scale="kaldi", triangularize_in_mel_space=True)
    win = window_function(400, "hamming", periodic=False)
    out = spectrogram(np.asarray(pcm, np.float32) * 2 ** 15, win, frame_length=400, hop_length=160, fft_length=512,
                      power=2.0, center=False, preemphasis=0.97, mel_filters=fb, log_mel="log",
                      mel_floor=1.192092955078125e-07, remove_dc_offset=True)
    return np.ascontiguousarray(out.T.astype(np.float32))   # [T][80]


def main():
    out = {}
    for ci, n in enumerate(ST.FIXTURE_LENGTHS):
        fb = hf_fbank(ST.audio(n, ci))
        assert fb.shape == (ST.n_frames(n), 80), fb.shape
        out[f"c{n}_frames"] = np.int32(fb.shape[0])
        out[f"c{n}_fbank"] = fb[fixture_rows(fb.shape[0])]
        print(n, fb.shape, float(fb.mean()), float(fb.std()))
    path = os.path.join(ROOT, "tests", "golden", "sensevoice_fbank.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
