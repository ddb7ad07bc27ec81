"""Measure SPT_MODEL_QUANT_RESIDENT: a large-v3 file with 2 encoder and 32 decoder layers in
q5_0, flag off against flag on, at B = 1 and B = 8.

The file is written from the oracle's tensors of a 2 + 2 model: decoder layer l takes layer l % 2's
tensors, quantised once each, so host memory stays at a few matrices (the values do not matter to the
times; the decoder's weight stream is the full model's, about 0.9 G weights).

    python scripts/bench_qresident.py [--reps 5] [--steps 64] [--out profiles/qresident/bench.json]
    python scripts/bench_qresident.py --one on --batch 1      # one setting (for a kernel-trace run)

A/B interleaved in one process: per repetition off, on, off, on ...; medians with min / max.  Reports
decode_ms / n_decode_passes, load time, weight_bytes and the residency.  bench.py is not involved."""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from oracle import ggml as G  # noqa: E402
from oracle import oracle as O  # noqa: E402


def write_file(path, n_dec=32, wtype=G.Q5_0):
    small = O.dims_for("large-v3", 2, 2)
    dims = O.dims_for("large-v3", 2, n_dec)
    base = O.Model(small, 1234, O.W_F32)
    src = base.tensors()
    base.close()
    vocab = G.synth_vocab(O.special_tokens(dims.n_vocab)["eot"])
    filters = np.ascontiguousarray(O.mel_filters(dims.n_mels), np.float32)
    raw_of = {}
    with open(path, "wb") as f:
        hp = [dims.n_vocab, dims.n_audio_ctx, dims.d, dims.n_head, dims.n_enc, dims.n_text_ctx, dims.d, dims.n_head,
              dims.n_dec, dims.n_mels, G.FTYPE[wtype] + 2000]
        f.write(struct.pack("<I", G.MAGIC) + struct.pack("<11i", *hp))
        f.write(struct.pack("<ii", *filters.shape) + filters.tobytes())
        f.write(struct.pack("<i", len(vocab)))
        for w in vocab:
            f.write(struct.pack("<I", len(w)) + w)
        for tid, name, ne in G.tensor_table(dims):
            stid = tid
            if tid >= 5000:   # decoder layer l -> layer l % 2 of the small model (32 ids per layer)
                layer, k = divmod(tid - 5000, 32)
                stid = 5000 + 32 * (layer % 2) + k
            ty = G.tensor_type(name, ne, wtype)
            if stid not in raw_of:
                raw_of[stid] = G.quantize(src[stid], ty)
            nb = name.encode()
            f.write(struct.pack("<iii", len(ne), len(nb), ty) + struct.pack(f"<{len(ne)}i", *ne) + nb)
            f.write(raw_of[stid])
    return dims


def load(path, resident, max_batch):
    from spittle_amd import WhisperEngine, WhisperModelParams
    t0 = time.perf_counter()
    e = WhisperEngine(WhisperModelParams(dtype="bf16", max_batch=max_batch, quant_resident=resident))
    e.load_model(path)
    return e, time.perf_counter() - t0


def pass_ms(e, batch, steps):
    from spittle_amd import WhisperInferenceParams
    p = WhisperInferenceParams(language="en", no_timestamps=True, temperature_inc=0.0, ignore_eot=True,
                               max_new_tokens=steps)
    e.transcribe_batch(batch, p)
    t = e.timings()
    return t["decode_ms"] / max(t["n_decode_passes"], 1)


def summary(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--dec", type=int, default=32)
    ap.add_argument("--one", choices=["off", "on"])
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--model", default=None, help="reuse a file written by an earlier run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch's HIP runtime first (as bench.py does)
    path = a.model or os.path.join(tempfile.gettempdir(), f"ggml-large-v3-e2-d{a.dec}-q5_0.bin")
    if not os.path.exists(path):
        t0 = time.perf_counter()
        write_file(path, a.dec)
        print(f"wrote {path}: {os.path.getsize(path) / 1e9:.3f} GB in {time.perf_counter() - t0:.1f} s", flush=True)
    audio = [O.synth_audio(i) for i in range(8)]
    if a.one:
        e, _ = load(path, a.one == "on", max(a.batch, 1))
        for _ in range(3):
            ms = pass_ms(e, audio[:a.batch], a.steps)
        print(json.dumps({"flag": a.one, "batch": a.batch, "pass_ms": ms}))
        return
    res = {"file_bytes": os.path.getsize(path), "steps": a.steps, "settings": {}}
    eng = {}
    for flag in ("off", "on"):
        eng[flag], lt = load(path, flag == "on", 8)
        res["settings"][flag] = {"load_s": lt, "weight_bytes": eng[flag].info()["weight_bytes"],
                                 "residency": eng[flag].weight_residency()}
        print(flag, res["settings"][flag], flush=True)
    for B in (1, 8):
        for flag in ("off", "on"):
            pass_ms(eng[flag], audio[:B], a.steps)   # warm-up: graphs captured, attributes set
        ms = {"off": [], "on": []}
        for _ in range(a.reps):
            for flag in ("off", "on"):
                ms[flag].append(pass_ms(eng[flag], audio[:B], a.steps))
        for flag in ("off", "on"):
            res["settings"][flag][f"pass_ms_B{B}"] = summary(ms[flag])
        print(f"B={B}", {k: summary(v) for k, v in ms.items()}, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
