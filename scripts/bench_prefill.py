"""Measure SPT_BLOCK_PREFILL: synthetic large-v3 (32 + 32 layers), bf16 and f16, one 5 s
utterance per batch row on the whisper_full path with timestamps, temperature_inc 0 (random weights would
otherwise fall back at every window), at most 32 tokens, prompt_tokens of P in {8, 16, 32, 64, 128, 224}
at B = 1 and B = 8.

    python scripts/bench_prefill.py [--reps 7] [--dtypes bf16,f16] [--out profiles/prefill/bench.json]
    python scripts/bench_prefill.py --one on --p 224 --batch 1 --dtype bf16     # one setting (kernel trace)

Flag off and on interleaved in one process and one context: per repetition off, on, off, on ...; median
and min-max of the call's wall time and of spt_call_stats.decode_ms, plus the prefill statistics.  The
flag-off call is the parent commit's path.  bench.py is not involved."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402

PS = (8, 16, 32, 64, 128, 224)


def params(n_prompt, flag, tokens):
    from spittle_amd import WhisperInferenceParams
    past = [int(v) for v in np.random.default_rng(11).integers(0, 50000, n_prompt)]
    return WhisperInferenceParams(language="en", temperature_inc=0.0, max_new_tokens=tokens, prompt_tokens=past,
                                  block_prefill=flag)


def call(e, audio, p):
    t0 = time.perf_counter()
    e.transcribe_batch(audio, p)
    wall = (time.perf_counter() - t0) * 1e3
    cs, ps = e.call_stats(), e.prefill_stats()
    return wall, cs["decode_ms"], cs["decoder_passes"], ps


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--ps", default=",".join(str(p) for p in PS))
    ap.add_argument("--spec", default="synthetic:large-v3")
    ap.add_argument("--one", choices=["off", "on"])
    ap.add_argument("--p", type=int, default=224)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch's HIP runtime first (as bench.py does)
    from spittle_amd import WhisperEngine, WhisperModelParams
    audio = [O.synth_audio(100 + i, 5 * 16000) for i in range(8)]
    if a.one:
        e = WhisperEngine(WhisperModelParams(dtype=a.dtype, max_batch=max(a.batch, 1)))
        e.load_model(a.spec)
        p = params(a.p, a.one == "on", a.tokens)
        for _ in range(3):
            wall, dec, passes, ps = call(e, audio[:a.batch], p)
        print(json.dumps({"flag": a.one, "dtype": a.dtype, "P": a.p, "batch": a.batch, "wall_ms": wall, "decode_ms": dec,
                          "decoder_passes": passes, "prefill": ps}))
        e.unload_model()
        return
    res = {"spec": a.spec, "tokens": a.tokens, "reps": a.reps, "rows": []}
    for dtype in a.dtypes.split(","):
        e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=8))
        e.load_model(a.spec)
        for B in [int(b) for b in a.batches.split(",")]:
            for P in [int(p) for p in a.ps.split(",")]:
                pp = {False: params(P, False, a.tokens), True: params(P, True, a.tokens)}
                for flag in (False, True):   # warm-up: graphs captured, attributes set, the workspace allocated
                    call(e, audio[:B], pp[flag])
                wall, dec, last = {False: [], True: []}, {False: [], True: []}, {}
                for _ in range(a.reps):
                    for flag in (False, True):
                        w, d, passes, ps = call(e, audio[:B], pp[flag])
                        wall[flag].append(w)
                        dec[flag].append(d)
                        last[flag] = {"decoder_passes": passes, "prefill": ps}
                row = {"dtype": dtype, "B": B, "P": P}
                for flag, name in ((False, "off"), (True, "on")):
                    row[name] = {"wall_ms": summary(wall[flag]), "decode_ms": summary(dec[flag]), **last[flag]}
                row["on_wins"] = row["on"]["decode_ms"]["max"] < row["off"]["decode_ms"]["min"]
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        e.unload_model()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print("RESULT " + line)


if __name__ == "__main__":
    main()
