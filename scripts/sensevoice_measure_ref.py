"""Measures, on the CPU, the numbers the SenseVoice tests' bars are set from (sensevoice-test-small with
the seeded weights of tests/sensevoice_torch.py), per audio case:

  * features: the engine stores no f16 before the first LayerNorm, so emulate_f16 against f32 is
    identically 0 there; the figure is the restatement's own f32 error against its f64 run
    (relative L2 and max-abs over the LFR rows after CMVN);
  * e_emul of the encoder output: sensevoice_torch(emulate_f16=True) against f32, relative L2 and max-abs;
  * the logit figure max |logit(emulate_f16) - logit(f32)|, bar_m = 4 x that, the share of rows whose
    f32 top-1 / top-2 margin is below bar_m, argmax mismatches between the two runs, and the blanks
    and repeated labels over the rows after the prefix.

    python scripts/sensevoice_measure_ref.py            # the table for E_EMUL in tests/test_gpu_sensevoice.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from tests import sensevoice_torch as ST  # noqa: E402


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def main():
    torch.set_num_threads(16)
    D = ST.TEST_SMALL
    W = ST.to_torch(ST.make_weights(D))
    cmvn = tuple(torch.from_numpy(v) for v in ST.make_cmvn(D))
    print("E_EMUL = {")
    notes = []
    for ci, n in enumerate(ST.CASES):
        pcm = ST.audio(n, ci)
        with torch.no_grad():
            f64 = ST.features(pcm, cmvn, D, torch.float64).numpy()
            ft, en, lg = (t.numpy() for t in ST.forward(W, cmvn, pcm, D, False))
            ft_e, en_e, lg_e = (t.numpy() for t in ST.forward(W, cmvn, pcm, D, True))
        assert np.array_equal(ft, ft_e)   # the front end is f32 in both
        d_emu = float(np.abs(lg_e - lg).max())
        mg = ST.margins(lg)
        ids = lg.argmax(axis=1)
        body = ids[D.n_prefix:]
        print(f"    {n}: ({rel_l2(ft, f64):.3e}, {np.abs(ft - f64).max():.3e}, {rel_l2(en_e, en):.3e}, "
              f"{np.abs(en_e - en).max():.3e}, {d_emu:.3e}),")
        notes.append(f"# n={n} R={len(ids)}: bar_m {4 * d_emu:.3e}, rows below {(mg < 4 * d_emu).mean():.3f}, argmax "
                     f"mismatches emu/f32 {(lg_e.argmax(axis=1) != ids).sum()}, blanks {(body == D.blank).sum()}, "
                     f"repeats {(body[1:] == body[:-1]).sum()}, logit std {lg.std():.2f}, tokens "
                     f"{len(ST.ctc_collapse(ids, D.n_prefix, D.blank)[1])}")
    print("}")
    print("\n".join(notes))


if __name__ == "__main__":
    main()
