"""Moonshine Base fp16 on the device: one JSON line.

Two shapes on synthetic:moonshine-base (seeded weights, so every row runs to its token limit):
  * b1: one 10 s clip, the app's shape -- wall latency (host clock around the call, which ends in a
    device synchronise), the engine's phase times, ms per decode step;
  * b64: 64 x 1 s windows in one call -- audio seconds per wall second (RTFx).
Each shape is warmed up (graph capture, code objects) and then timed `--repeats` times; the median
and the min / max are reported.  The baseline in the same line is the torch f32 restatement
(tests/moonshine_torch.py, random weights of the same geometry) on 16 CPU threads: stem + encoder
+ a greedy loop with K/V caches of the same number of steps for the 10 s clip.  No device: the script fails.

    python scripts/bench_moonshine.py [--repeats 10] [--warmup 3] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "repeats": repeats}


def step_bytes(info, n_keys_self, n_keys_cross):
    """bytes one decode step must stream at B = 1: the decoder's f16 weights (tied embedding included,
    read once for the logits) and the f16 K/V it attends over"""
    d, ff, L, V = info["d"], info["ff"], info["n_dec_layers"], info["n_vocab"]
    per_layer = (3 * d * d + d * d) + (d * d + d * d) + 2 * ff * d + d * ff
    kv = L * 2 * d * (n_keys_self + n_keys_cross)
    return 2 * (L * per_layer + V * d + kv)


def cpu_greedy_cached(MT, W, enc, D, n_steps):
    """torch f32 greedy decoding with self and cross K/V caches: one new token's work per step"""
    import torch
    import torch.nn.functional as F
    Te = enc.shape[0]
    emb = W["model.decoder.embed_tokens.weight"]
    cross, selfkv = [], []
    for l in range(D.n_dec):
        p = f"model.decoder.layers.{l}.encoder_attn."
        cross.append(((enc @ W[p + "k_proj.weight"].T).view(Te, D.H, D.dh), (enc @ W[p + "v_proj.weight"].T).view(Te, D.H, D.dh)))
        selfkv.append([torch.zeros(0, D.H, D.dh), torch.zeros(0, D.H, D.dh)])
    toks = [D.bos]
    for step in range(n_steps):
        x = emb[toks[-1]][None]
        cos, sin = MT._rope_tables(D, torch.tensor([step]))
        for l in range(D.n_dec):
            p = f"model.decoder.layers.{l}."
            xn = MT._ln(x, W[p + "input_layernorm.weight"])
            q, k, v = (xn @ W[p + f"self_attn.{n}_proj.weight"].T for n in "qkv")
            q = MT._rope(q.view(1, D.H, D.dh), cos, sin, D.rot)
            selfkv[l][0] = torch.cat((selfkv[l][0], MT._rope(k.view(1, D.H, D.dh), cos, sin, D.rot)))
            selfkv[l][1] = torch.cat((selfkv[l][1], v.view(1, D.H, D.dh)))
            x = x + MT._attend(q, selfkv[l][0], selfkv[l][1], D, None, False, False) @ W[p + "self_attn.o_proj.weight"].T
            xn = MT._ln(x, W[p + "post_attention_layernorm.weight"])
            q = (xn @ W[p + "encoder_attn.q_proj.weight"].T).view(1, D.H, D.dh)
            x = x + MT._attend(q, cross[l][0], cross[l][1], D, None, False, False) @ W[p + "encoder_attn.o_proj.weight"].T
            xn = MT._ln(x, W[p + "final_layernorm.weight"])
            h, gate = (xn @ W[p + "mlp.fc1.weight"].T + W[p + "mlp.fc1.bias"]).chunk(2, dim=-1)
            x = x + (F.silu(gate) * h) @ W[p + "mlp.fc2.weight"].T + W[p + "mlp.fc2.bias"]
        toks.append(int((MT._ln(x, W["model.decoder.norm.weight"]) @ emb.T)[0].argmax()))
    return toks[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_moonshine: no GPU (this measurement has no CPU fallback)")
    from spittle_amd import MoonshineEngine, MoonshineModelParams
    from tests import moonshine_torch as MT

    out = {"model": "synthetic:moonshine-base", "dtype": "f16", "device": torch.cuda.get_device_name(0)}
    clip = MT.audio(160000, 3)
    e = MoonshineEngine()
    mp = MoonshineModelParams.variant("base")
    mp.max_batch, mp.max_samples = 1, 160000
    e.load_model_with_params("synthetic:moonshine-base", mp)
    info = e.info()
    r = timed(lambda: e.transcribe_samples(clip), a.warmup, a.repeats)
    tm = e.timings()
    res = e.transcribe_samples(clip)
    steps = tm["n_steps"]
    t3 = MT.frame_counts(160000)[2]
    sb = step_bytes(info, steps / 2, t3)
    out["b1_10s"] = dict(r, tokens=len(res.tokens), n_steps=steps, stem_ms=tm["stem_ms"], encoder_ms=tm["encoder_ms"],
                         cross_kv_ms=tm["cross_kv_ms"], decode_ms=tm["decode_ms"], ms_per_step=tm["decode_ms"] / max(steps, 1),
                         step_bytes=sb, step_floor_us_at_8TBs=sb / 8e12 * 1e6, rtfx=10.0 / (r["median_ms"] / 1e3))
    e.unload_model()

    wins = [MT.audio(16000, 100 + i) for i in range(64)]
    mp.max_batch, mp.max_samples = 64, 16000
    e.load_model_with_params("synthetic:moonshine-base", mp)
    r = timed(lambda: e.transcribe_batch(wins), a.warmup, a.repeats)
    tm = e.timings()
    out["b64_1s"] = dict(r, n_steps=tm["n_steps"], stem_ms=tm["stem_ms"], encoder_ms=tm["encoder_ms"],
                         cross_kv_ms=tm["cross_kv_ms"], decode_ms=tm["decode_ms"], rtfx=64.0 / (r["median_ms"] / 1e3))
    e.unload_model()

    if not a.no_cpu:
        torch.set_num_threads(16)
        D = MT.Dims(416, 8, 1664, 8, 8, 32768)
        W = MT.to_torch(MT.make_weights(D, 1, 0.03))
        with torch.no_grad():
            t0 = time.perf_counter()
            enc = MT.encoder(W, MT.stem(W, clip, D), D)
            t1 = time.perf_counter()
            toks = cpu_greedy_cached(MT, W, enc, D, MT.max_tokens(160000))
            t2 = time.perf_counter()
        out["cpu_torch_f32_16t_10s"] = {"encoder_ms": (t1 - t0) * 1e3, "decode_ms": (t2 - t1) * 1e3,
                                        "total_ms": (t2 - t0) * 1e3, "steps": len(toks),
                                        "note": "greedy loop with self and cross K/V caches"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
