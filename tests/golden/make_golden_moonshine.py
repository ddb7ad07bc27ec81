"""Writes tests/golden/moonshine_small.npz and moonshine_tiny2.npz from HF transformers'
MoonshineForConditionalGeneration (a local config, no download) loaded with the seeded weights of
tests/moonshine_torch.make_weights.  Per audio case (tests/moonshine_torch.CASES): rows of the stem
output and of the encoder output (moonshine_torch.fixture_rows), HF's own greedy tokens (argmax from
<s>, ceil(6.5 n / 16000) steps at most) and the teacher-forced logits over them.

    python tests/golden/make_golden_moonshine.py

The tests never import transformers; only this script does."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import moonshine_torch as MT  # noqa: E402


def hf_model(D, weights):
    from transformers import MoonshineConfig, MoonshineForConditionalGeneration
    cfg = MoonshineConfig(vocab_size=D.vocab, hidden_size=D.d, intermediate_size=D.ff,
                          encoder_num_hidden_layers=D.n_enc, decoder_num_hidden_layers=D.n_dec,
                          encoder_num_attention_heads=D.H, decoder_num_attention_heads=D.H,
                          bos_token_id=D.bos, eos_token_id=D.eos, decoder_start_token_id=D.bos)
    cfg._attn_implementation = "eager"
    m = MoonshineForConditionalGeneration(cfg).eval()
    sd = m.state_dict()
    ours = dict(weights)
    ours["proj_out.weight"] = weights["model.decoder.embed_tokens.weight"]
    assert set(sd) == set(ours), (sorted(set(sd) - set(ours)), sorted(set(ours) - set(sd)))
    for k, v in ours.items():
        assert tuple(sd[k].shape) == v.shape, (k, sd[k].shape, v.shape)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ours.items()})
    rot = int((D.d // D.H) * cfg.rope_parameters.get("partial_rotary_factor", 1.0))
    assert rot == D.rot, (rot, D.rot)
    return m


@torch.no_grad()
def run_case(m, D, n, seed):
    from transformers.models.moonshine.modeling_moonshine import MoonshineEncoderModelOutput as BaseModelOutput
    x = torch.from_numpy(MT.audio(n, seed))[None]
    enc_mod = m.model.encoder
    h = torch.tanh(enc_mod.conv1(x.unsqueeze(1)))
    h = enc_mod.groupnorm(h)
    h = torch.nn.functional.gelu(enc_mod.conv2(h))
    h = torch.nn.functional.gelu(enc_mod.conv3(h))
    stem = h[0].T.contiguous()
    enc = enc_mod(x).last_hidden_state
    assert enc.shape[1] == MT.frame_counts(n)[2], (enc.shape, n)
    toks = [D.bos]
    hit = False
    for _ in range(MT.max_tokens(n)):
        lg = m(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=torch.tensor([toks])).logits[0, -1]
        t = int(lg.argmax())
        if t == D.eos:
            hit = True
            break
        toks.append(t)
    logits = m(encoder_outputs=BaseModelOutput(last_hidden_state=enc),
               decoder_input_ids=torch.tensor([toks[:-1] if len(toks) > 1 else toks])).logits[0]
    rows = MT.fixture_rows(enc.shape[1])
    return {"stem": stem[rows].numpy(), "enc": enc[0][rows].numpy(), "tokens": np.array(toks[1:], np.int32),
            "logits": logits.numpy().astype(np.float32), "hit_eos": np.array(int(hit), np.int32)}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(16)
    for name, (D, _spec, seed, std) in MT.FIXTURES.items():
        m = hf_model(D, MT.make_weights(D, seed, std))
        out = {"seed": np.array(seed), "std": np.array(std, np.float64)}
        for ci, n in enumerate(MT.CASES):
            r = run_case(m, D, n, ci)
            mg = MT.margins(r["logits"])
            print(name, n, "T3", MT.frame_counts(n)[2], "tokens", len(r["tokens"]), "distinct", len(set(r["tokens"].tolist())),
                  "hit_eos", int(r["hit_eos"]), "margin min/median %.3f %.3f" % (mg.min(), np.median(mg)))
            for k, v in r.items():
                out[f"c{n}_{k}"] = v
        path = os.path.join(ROOT, "tests", "golden", name + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
