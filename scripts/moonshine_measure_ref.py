"""Measures, on the CPU, the numbers the Moonshine tests' bars are set from:

  * tests/moonshine_torch (f32) against the HF fixtures: stem / encoder / logits error, token agreement;
  * e_emul: moonshine_torch(emulate_f16=True) against the f32 fixture (relative L2 and max-abs);
  * bar_m = 4 x max |logit(emulate_f16) - logit(f32)| and the share of decode steps whose
    reference top-1 / top-2 margin is below it.

    python scripts/moonshine_measure_ref.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from tests import moonshine_torch as MT  # noqa: E402


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def main():
    torch.set_num_threads(16)
    for name, (D, _spec, seed, std) in MT.FIXTURES.items():
        fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        W = MT.to_torch(MT.make_weights(D, seed, std))
        for ci, n in enumerate(MT.CASES):
            pcm = MT.audio(n, ci)
            rows = MT.fixture_rows(MT.frame_counts(n)[2])
            toks = fx[f"c{n}_tokens"]
            prefix = [D.bos] + list(toks[:-1])
            out = {}
            with torch.no_grad():
                for emu in (False, True):
                    st = MT.stem(W, pcm, D, emu)
                    en = MT.encoder(W, st, D, emu)
                    lg = MT.decoder_logits(W, en, prefix, D, emu)
                    out[emu] = (st[rows].numpy(), en[rows].numpy(), lg.numpy())
                g, hit, _ = MT.greedy(W, MT.encoder(W, MT.stem(W, pcm, D), D), D, MT.max_tokens(n))
            f = (fx[f"c{n}_stem"], fx[f"c{n}_enc"], fx[f"c{n}_logits"])
            mg = MT.margins(f[2])
            d_emu = float(np.abs(out[True][2] - out[False][2]).max())
            print(f"{name} n={n}: f32 vs HF max-abs stem {np.abs(out[False][0] - f[0]).max():.2e} enc "
                  f"{np.abs(out[False][1] - f[1]).max():.2e} logits {np.abs(out[False][2] - f[2]).max():.2e} "
                  f"tokens_equal {list(g) == list(toks)}")
            print(f"    e_emul stem rel {rel_l2(out[True][0], f[0]):.3e} max {np.abs(out[True][0] - f[0]).max():.3e} | "
                  f"enc rel {rel_l2(out[True][1], f[1]):.3e} max {np.abs(out[True][1] - f[1]).max():.3e} | "
                  f"logits emu-f32 max {d_emu:.3e} bar_m {4 * d_emu:.3e} steps below {(mg < 4 * d_emu).mean():.3f} "
                  f"first below {int(np.argmax(mg < 4 * d_emu)) if (mg < 4 * d_emu).any() else -1} of {len(mg)}")


if __name__ == "__main__":
    main()
