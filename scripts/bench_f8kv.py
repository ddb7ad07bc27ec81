"""Measure SPT_MODEL_CROSS_KV_F8: large-v3 geometry (synthetic weights, 2 encoder layers, 32
decoder layers), bf16, flag off against flag on, at B = 1 and B = 8.

    python scripts/bench_f8kv.py [--reps 7] [--steps 64] [--out profiles/f8kv/bench.json]
    python scripts/bench_f8kv.py --one on --batch 8      # one setting (for a kernel-trace run)

A/B interleaved in one process: per repetition off, on, off, on ...; medians with min / max.  Reports the
workspace and cross K/V bytes, cross_kv_ms (the per-group GEMMs plus the quantiser against the single GEMM)
and decode_ms / n_decode_passes.  bench.py is not involved.  Run the GPU step under `timeout`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402


def load(spec, f8, max_batch):
    from spittle_amd import WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype="bf16", max_batch=max_batch, cross_kv_f8=f8))
    e.load_model(spec)
    return e


def run(e, batch, steps):
    """-> (ms per decode pass, cross_kv_ms) of one call"""
    from spittle_amd import WhisperInferenceParams
    p = WhisperInferenceParams(language="en", no_timestamps=True, temperature_inc=0.0, ignore_eot=True,
                               max_new_tokens=steps)
    e.transcribe_batch(batch, p)
    t = e.timings()
    return t["decode_ms"] / max(t["n_decode_passes"], 1), t["cross_kv_ms"]


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--dec", type=int, default=32)
    ap.add_argument("--one", choices=["off", "on"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch's HIP runtime first (as bench.py does)
    spec = f"synthetic:large-v3:enc=2:dec={a.dec}"
    audio = [O.synth_audio(i) for i in range(8)]
    if a.one:
        e = load(spec, a.one == "on", max(a.batch, 1))
        for _ in range(3):
            ms, kv = run(e, audio[:a.batch], a.steps)
        print(json.dumps({"flag": a.one, "batch": a.batch, "pass_ms": ms, "cross_kv_ms": kv}))
        return
    res = {"spec": spec, "steps": a.steps, "settings": {}}
    eng = {}
    for flag in ("off", "on"):
        eng[flag] = load(spec, flag == "on", 8)
        res["settings"][flag] = {"workspace_bytes": eng[flag].info()["workspace_bytes"], "cross_kv": eng[flag].cross_kv_info()}
        print(flag, res["settings"][flag], flush=True)
    for B in (1, 8):
        for flag in ("off", "on"):
            run(eng[flag], audio[:B], a.steps)   # warm-up: graphs captured, attributes set
        ms = {"off": [], "on": []}
        kv = {"off": [], "on": []}
        for _ in range(a.reps):
            for flag in ("off", "on"):
                m, k = run(eng[flag], audio[:B], a.steps)
                ms[flag].append(m)
                kv[flag].append(k)
        for flag in ("off", "on"):
            res["settings"][flag][f"pass_ms_B{B}"] = summary(ms[flag])
            res["settings"][flag][f"cross_kv_ms_B{B}"] = summary(kv[flag])
        print(f"B={B} pass_ms", {k: summary(v) for k, v in ms.items()}, flush=True)
        print(f"B={B} cross_kv_ms", {k: summary(v) for k, v in kv.items()}, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
