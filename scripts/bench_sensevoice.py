"""SenseVoice-Small fp16 on the device: one JSON line.

Three shapes on synthetic:sensevoice-small (seeded weights, full depth: 1 + 49 + 20 layers):
  * b1_10s: one 10 s clip (R = 171 rows), the app's shape -- wall latency (host clock around the
    call, which ends in a device synchronise) and the engine's phase times;
  * b1_30s: one 30 s clip (R = 504);
  * b64_1s: 64 x 1 s windows in one call -- audio seconds per wall second (RTFx).
Each shape is warmed up and then timed `--repeats` times; the median and the min / max are reported,
next to the floors the pass is held against: the f16 weight bytes streamed once at 8 TB/s, and the
GEMM flops of the rows.  The baseline in the same line is the torch f32 restatement
(tests/sensevoice_torch.py, random weights of the same geometry) on 16 CPU threads.  No device: the
script fails.

    python scripts/bench_sensevoice.py [--repeats 10] [--warmup 3] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def gemm_flops(info, rows):
    """multiply-adds x 2 of the GEMMs (and the attention's two products) for `rows` encoder rows of one utterance"""
    d, ff, V, k0 = info["d"], info["ff"], info["n_vocab"], info["input_dim"]
    layers = info["n_enc0_layers"] + info["n_enc_layers"] + info["n_tp_layers"]
    per_row = layers * (3 * d * d + d * d + 2 * d * ff + 2 * rows * d) + 3 * d * (k0 - d) + V * d
    return 2.0 * rows * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sensevoice: no GPU (this measurement has no CPU fallback)")
    from spittle_amd import Language, SenseVoiceEngine, SenseVoiceInferenceParams, SenseVoiceModelParams
    from tests import sensevoice_torch as ST

    out = {"model": "synthetic:sensevoice-small", "dtype": "f16", "device": torch.cuda.get_device_name(0)}
    ip = SenseVoiceInferenceParams(language=Language.English, use_itn=True)   # what the app sends
    e = SenseVoiceEngine()
    clips = {}
    for name, n in (("b1_10s", 160000), ("b1_30s", 480000)):
        clips[name] = clip = ST.audio(n, 3)
        e.load_model_with_params("synthetic:sensevoice-small", SenseVoiceModelParams(max_batch=1, max_samples=n))
        info = e.info()
        r = timed(lambda: e.transcribe_samples(clip, ip), a.warmup, a.repeats)
        tm = e.timings()
        res = e.transcribe_samples(clip, ip)
        fl = gemm_flops(info, tm["rows"])
        wb = info["weight_bytes"]
        out[name] = dict(r, rows=tm["rows"], tokens=len(res.tokens), frontend_ms=tm["frontend_ms"], encoder_ms=tm["encoder_ms"],
                         ctc_ms=tm["ctc_ms"], device_ms=tm["total_ms"], weight_bytes=wb,
                         weight_floor_us_at_8TBs=wb / 8e12 * 1e6, gemm_tflop=fl / 1e12,
                         achieved_tflops=fl / 1e12 / (tm["total_ms"] / 1e3), rtfx=(n / 16000.0) / (r["median_ms"] / 1e3))
        e.unload_model()

    wins = [ST.audio(16000, 100 + i) for i in range(64)]
    e.load_model_with_params("synthetic:sensevoice-small", SenseVoiceModelParams(max_batch=64, max_samples=16000))
    info = e.info()
    r = timed(lambda: e.transcribe_batch(wins, ip), a.warmup, a.repeats)
    tm = e.timings()
    fl = 64 * gemm_flops(info, tm["rows"])
    out["b64_1s"] = dict(r, rows=tm["rows"], frontend_ms=tm["frontend_ms"], encoder_ms=tm["encoder_ms"], ctc_ms=tm["ctc_ms"],
                         device_ms=tm["total_ms"], gemm_tflop=fl / 1e12, achieved_tflops=fl / 1e12 / (tm["total_ms"] / 1e3),
                         rtfx=64.0 / (r["median_ms"] / 1e3))
    e.unload_model()

    if not a.no_cpu:
        torch.set_num_threads(16)
        D = ST.SMALL
        W = ST.to_torch(ST.make_weights(D, 1))
        cm = tuple(torch.from_numpy(v) for v in ST.make_cmvn(D, 1))
        for name in ("b1_10s", "b1_30s"):
            with torch.no_grad():
                ST.forward(W, cm, clips[name][:16000], D)   # warm the thread pool
                t0 = time.perf_counter()
                ft = ST.features(clips[name], cm, D)
                t1 = time.perf_counter()
                en = ST.encoder(W, ST.input_rows(W, ft, D, 2, True), D)
                t2 = time.perf_counter()
                ids = ST.ctc_logits(W, en).argmax(dim=1)
                t3 = time.perf_counter()
            out["cpu_torch_f32_16t_" + name[3:]] = {"frontend_ms": (t1 - t0) * 1e3, "encoder_ms": (t2 - t1) * 1e3,
                                                    "ctc_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3, "rows": int(ids.numel())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
