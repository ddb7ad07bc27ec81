"""Generate tests/golden/tiny_en_align.npz: HF transformers' token alignment of a seeded synthetic
model, the pin of tests/test_gpu_align_engine.py (run in the build container only; the GPU box never
imports transformers or this script).

The model is make_golden.py's: a LOCAL WhisperConfig holding the oracle's seeded tensors of
synthetic:tiny.en:enc=2:dec=2, here with attn_implementation="eager" so the decoder returns its
cross-attention probabilities.  Per case (5 s and 30 s of oracle.synth_audio(0)): the greedy
no-timestamp tokens (make_golden.py's loop), then ONE teacher-forced pass of [sot, <|notimestamps|>,
text ...] in float32 and in float64.  HF's WhisperEncoder applies the erf GELU to its two convolutions
whatever activation_function says; whisper.cpp, the oracle and the engine use the tanh form there as
everywhere else ("GELU: tanh vs erf"), and that alone moves the encoder output by 1.9e-4
relative L2 and p by 1.4e-3.  So the encoder runs here with the stem's GELU in the tanh form too
(stem_tanh), which brings HF's encoder within 1e-6 of the oracle's (asserted below): the fixture then
holds the function the engine computes, and p_noise stays HF's own float32 - float64 difference.
Stored: the tokens, the alignment heads' probabilities (every head of the top half of the decoder layers, rows from <|notimestamps|> on, the first M = n_frames / 2
keys, softmax taken over all 1500), HF's matrix (_extract_token_timestamps' normalise + _median_filter
+ head mean) and its _dynamic_time_warping path, and p_noise: the largest relative difference between
the float32 and the float64 probabilities -- the reference's own error, from which the test's bar is
8 x p_noise.

Usage:  python tests/golden/make_golden_align.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, HERE)

from oracle import oracle as O  # noqa: E402
import make_golden as G  # noqa: E402

CASES = {"s5": (80000, 3), "s30": (480000, 11)}  # samples, text tokens (the replay crosses a 4-row chunk at 11)


def build(dims, tensors, dtype):
    from transformers import WhisperConfig, WhisperModel
    cfg = WhisperConfig(vocab_size=dims.n_vocab, num_mel_bins=dims.n_mels, d_model=dims.d,
                        encoder_layers=dims.n_enc, decoder_layers=dims.n_dec,
                        encoder_attention_heads=dims.n_head, decoder_attention_heads=dims.n_head,
                        encoder_ffn_dim=4 * dims.d, decoder_ffn_dim=4 * dims.d,
                        max_source_positions=dims.n_audio_ctx, max_target_positions=dims.n_text_ctx,
                        activation_function="gelu_new", dropout=0.0, attention_dropout=0.0,
                        activation_dropout=0.0, attn_implementation="eager")
    model = WhisperModel(cfg).eval()
    sd = model.state_dict()
    names = G.hf_name_map(dims.n_enc, dims.n_dec)
    model.load_state_dict({names[t]: torch.from_numpy(a.reshape(tuple(sd[names[t]].shape))) for t, a in tensors.items()},
                          strict=True)
    return model.to(dtype)


class stem_tanh:
    """Within the block, nn.functional.gelu -- which WhisperEncoder.forward calls on conv1 and conv2 only --
    is the tanh form (the decoder and encoder layers take gelu_new from ACT2FN and are not touched)."""

    def __enter__(self):
        self.orig = torch.nn.functional.gelu
        torch.nn.functional.gelu = lambda t, *a, **k: self.orig(t, approximate="tanh")

    def __exit__(self, *exc):
        torch.nn.functional.gelu = self.orig


@torch.no_grad()
def encode(model, mel):
    dt = next(model.parameters()).dtype
    with stem_tanh():
        return model.encoder(torch.from_numpy(mel)[None].to(dt)).last_hidden_state


@torch.no_grad()
def probs(model, mel, ids, dims, M):
    """The alignment heads' probabilities [A][N][M] of one teacher-forced pass (rows from <|notimestamps|> on)."""
    enc = encode(model, mel)
    out = model.decoder(input_ids=torch.tensor([ids]), encoder_hidden_states=enc, output_attentions=True)
    heads = [out.cross_attentions[l][0, h] for l in range(dims.n_dec // 2, dims.n_dec) for h in range(dims.n_head)]
    n_skip = len(O.default_prompt(dims.n_vocab)) - 1
    return torch.stack(heads)[:, n_skip:, :M]


@torch.no_grad()
def greedy(model, mel, dims, n):
    enc = encode(model, mel)
    toks, out = list(O.default_prompt(dims.n_vocab)), []
    for s in range(n):
        h = model.decoder(input_ids=torch.tensor([toks]), encoder_hidden_states=enc).last_hidden_state
        lg = (h[0, -1] @ model.decoder.embed_tokens.weight.T).numpy().astype(np.float32)
        sl = G.suppress_np(lg, dims.n_vocab, s == 0)
        o = np.argsort(-sl)[:2]
        out.append((int(o[0]), float(sl[o[0]] - sl[o[1]])))
        toks.append(int(o[0]))
    return out


def main():
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter
    dims = O.dims_for("tiny.en", 2, 2)
    om = O.Model(dims, 1234, O.W_F32)
    tensors = om.tensors()
    m32, m64 = build(dims, tensors, torch.float32), build(dims, tensors, torch.float64)
    sp = O.special_tokens(dims.n_vocab)
    save = dict(dims=np.array([dims.n_enc, dims.n_dec, dims.n_head], np.int32), seed=np.int64(1234), audio=np.int32(0))
    noise = 0.0
    for name, (n_samples, n_text) in CASES.items():
        x = O.synth_audio(0, n_samples)
        mel = O.mel_window(O.mel_full(x, dims.n_mels), 0)
        h64 = encode(m64, mel)[0].numpy()
        gap = float(np.linalg.norm(om.encode(mel) - h64) / np.linalg.norm(h64))
        assert gap < 5e-6, gap  # the same encoder as the oracle's (1.9e-4 with HF's erf stem)
        got = greedy(m32, mel, dims, n_text)
        toks = [t for t, _ in got]
        assert all(t < sp["eot"] for t in toks), toks
        n_frames = min(3000, 1 + (n_samples + 200 - 400) // 160)
        M = n_frames // 2
        ids = list(O.default_prompt(dims.n_vocab)) + toks
        p32, p64 = probs(m32, mel, ids, dims, M), probs(m64, mel, ids, dims, M)
        noise = max(noise, float(((p32.double() - p64).abs() / p64).max()))
        w = p32.double()
        z = (w - w.mean(-2, keepdim=True)) / torch.std(w, dim=-2, keepdim=True, unbiased=False)
        m = _median_filter(z, 7).mean(0)
        ti, tj = _dynamic_time_warping(-m.numpy())
        save.update({f"{name}_n_samples": np.int32(n_samples), f"{name}_tokens": np.int32(toks),
                     f"{name}_gaps": np.float32([g for _, g in got]), f"{name}_p": p32.numpy().astype(np.float32),
                     f"{name}_m": m.numpy(), f"{name}_path": np.stack([ti, tj], 1).astype(np.int32)})
        print(name, "tokens", toks, "smallest top-2 gap", min(g for _, g in got), "M", M, "path", len(ti))
    save["p_noise"] = np.float64(noise)
    path = os.path.join(HERE, "tiny_en_align.npz")
    np.savez_compressed(path, **save)
    print("p_noise", noise, "->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
